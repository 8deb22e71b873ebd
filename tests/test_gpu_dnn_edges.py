"""The kernels every DNN training step runs (tfkaldi_amd/csrc/kernels.hip and the statistics epilogue of the forward GEMMs) at
their own edges, each against a float64 reference evaluated on the DEVICE's own fp32 input of the kernel under test, so that the
comparison sees that kernel's round-off alone (the isolation of tests/test_gpu_ctc_edges.py).  One "dnn-edges" line per case
under `pytest -s`, headed by the library's build id (recorded in profiles/dnn_kernel_edges.txt).

A. softmax_xent_kernel<NV>, the TRAINING kernel: every register width NV = 1 / 2 / 4 / 8 full and one float4 past it, tails of 1,
   2 and 3 live columns, the generic kernel (the only one that writes the operand twin element by element), labels in column 0,
   column O - 1 and every slot of the last live float4; the net as initialised and a peaked one (every row's logits spread over
   more than 110, labels on columns whose expf underflows).  The net (tanh, no batch norm, no dropout) gives the same logits in
   the evaluation and the training pass: eval_accumulate first -- DBG_LOGITS then holds the logits `zdev`, its loss is compared
   with the float64 log-sum-exp on zdev BEFORE the training pass -- accumulate second, after which DBG_LOGITS holds dLogits
   (float64 softmax(zdev) - onehot).  Guard of the equivalence: BATCH_LOSS of the two passes to rtol 1e-6.  Every gradient is
   compared with OracleDNN.backward_from_dlogits fed the float64 dLogits: the output layer's W and b gradients are computed from
   the operand twin of dLogits (emulated fp32: three bf16 planes, bfloat16: one), so they prove that the twin was written right.
   The stacked case runs on a ReLU + batch-norm net, the only chain tfk_accumulate_stacked stacks (engine.hip: stack_eligible;
   any other chain would run its segments one after the other and never see a padding row).
B. Batch-norm statistics forward and backward: DBG_PREACT / DBG_BN_MEAN / DBG_BN_RSTD / DBG_HIDDEN of each layer after
   accumulate, against float64 column statistics of the device's own pre-activation.  H = 130: two 128-column blocks, the second
   with two live columns.  Chains: relu + BN (fused EPI_COLSTATS forward, EPI_DACT backward); tanh + BN + L2Norm, the chain that
   runs the OTHER statistics code -- bn_stats_partial_kernel / bn_stats_final_kernel forward and hb_stats_kernel backward
   (engine.hip: an L2 chain takes neither fused path; sigmoid + BN alone still takes EPI_DACT, only sigmoid + BN + dropout would
   not); relu + BN + dropout at three row counts.  Row counts: a last chunk of one row, exactly 16 / 17 / 32 / 33 chunks of 128
   rows, ragged 16- and 32-row splits.  Besides ordinary data an OFFSET variant: layer 0 has |mean| = 30 on every other column
   at a spread of about one (a one-pass variance or a wrong chunk count in the merge is off by 1e-4 .. 1e-2 there,
   tests/test_bn_stats_model.py), and one column with zero weights (and beta = 0.25, so that a ReLU shows its output) whose
   variance is exactly 0: its mean must be the bias bit for bit, because rstd = 1 / sqrt(eps) = 31.6 turns one ulp of 30 into
   6e-5 of the output.  (A mean formed as sum * (1 / n) misses that at 26 and at 63 rows; the kernels divide.)
   The oracle that checks the gradients is evaluated on the device's pre-activations as well (its hidden affine products are
   replaced by zdev): where two of two or three rows nearly agree in a column, rstd amplifies the ulp of 30 by which the
   device's z differs from a float64 product, twice over two layers -- a property of the data, not of a kernel; the
   contractions have their own tests.
   Bound on mean and rstd: 4x the error of the fp32 reference MODEL (test_bn_stats_model.bn_stats_model: sequential sums per chunk,
   sequential Chan merge -- the worst order the device could use) against float64 on the same zdev, floored at one fp32 ulp of
   the reference value; the factor 4 covers a different but still correct summation order.  Round-off of a column sum scales
   with the magnitude of what is summed, so the model's error is taken relative to max |z| of its column (mean) or to rstd, the
   worst column of the case sets the figure, and every device column is held to 4x that figure times its own scale.  The
   model's chunk is the kernel's: 128 rows (emulated fp32), the stricter of 64 / 128 (the other two arithmetics' tiles), or the
   rows per block of bn_stats_partial_kernel (L2 chain).  eps is the fp32 value the kernels add (float32(1e-3)).
   ReLU chains: the oracle runs with the engine's on/off pattern (OracleDNN's relu_active hook, as tests/test_gpu_full_size.py);
   the patterns may differ only within 1e-4 of the kink (fp32 ulp of 30 is 1.9e-6, a few of them through rstd ~ 1) on fewer than
   1e-4 of the units (or on one); bfloat16: within 1e-2 on fewer than 1e-3 (a bf16 operand of layer 1 that rounds the other way moves a
   pre-activation by up to 2^-8 of one product).
C. adam_kernel on the values where it can go wrong -- the clip boundary and its fp32 neighbours, zero and signed zero, squares
   that underflow, the fp32 maximum -- with the moments compared as well as the parameters, and the operand twins the kernel
   writes with the update compared with twins rebuilt from the parameters.

Tolerances are the project's own (tests/test_gpu_engine_parity.py): dLogits rtol 1e-4 + atol 2e-6, loss rtol 2e-5, hidden outputs
rtol 1e-4 + atol 2e-5, gradients _check_grads' rule, moving averages rtol 1e-5 + atol 1e-6, Adam rtol 1e-5 + atol 2e-6; bfloat16
gradients: relative Frobenius error <= 2e-3 and loss rtol 5e-4 (tests/test_gpu_bf16_mode.py), a zero reference under
_check_grads' absolute term."""
import numpy as np
import pytest

from oracle.dnn_oracle import OracleDNN, _nonlin
from oracle.dnn_oracle import bn_stat_bounds as _stat_bounds  # (the link checker, tests/test_gpu_bf16_links.py, bounds F2 with it too)
from test_bn_stats_model import BN_EPS, CONSTANT_COL, bn_stats_model, offset_layer, stats64
from test_gpu_engine_parity import _check_grads
from util import assert_close, batch, copy_oracle_to_engine, engine_grads, engine_params, oracle_kwargs, randomize

pytestmark = pytest.mark.gpu


def _engine(kw, dtype):
    from tfkaldi_amd import _lib
    from tfkaldi_amd.engine import Engine
    return Engine(_lib.make_config(max_frames=kw["max_frames"], seed=1234, compute_dtype=dtype, **oracle_kwargs(kw)))


class _Oracle(OracleDNN):
    """OracleDNN whose hidden layers can be evaluated on the DEVICE's pre-activations: with `zdev` set (one [T, H] array per
    hidden layer) the forward product of hidden layer l is replaced so that z = zdev[l]; everything else is the oracle's own"""
    zdev = None

    def _mm(self, a, b):
        if self.zdev is not None:
            for l in range(self.L):
                if b is self.W[l]:  # (_forward passes the matrix itself, backward its transpose)
                    return self.zdev[l].astype(np.float64) - self.b[l]
        return OracleDNN._mm(self, a, b)


def _oracle(kw, dtype, rng, **over):
    oracle = _Oracle(gemm_dtype="bfloat16" if dtype == "bfloat16" else "float32", **dict(oracle_kwargs(kw), **over))
    randomize(oracle, rng)
    return oracle


@pytest.fixture(scope="module")
def nets(gpu):
    """engines by (arithmetic, shape), made on first use, shared by the cases of this file and closed at its end; every case
    loads its own parameters"""
    from tfkaldi_amd.build import library_id
    print("\ndnn-edges build id %s" % library_id())
    made = {}

    def get(dtype, **kw):
        key = (dtype,) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = _engine(kw, dtype)
        return made[key]
    yield get
    for eng in made.values():
        eng.close()


def _rel(got, want):
    return abs(got - want) / max(abs(want), 1e-30)


def _rel_fro(got, want):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / max(np.linalg.norm(want), 1e-30))


def _dead_bias(oracle, k):
    return oracle.bn and k.startswith("b") and not k.startswith("beta") and k != "b%d" % oracle.L


def _grads_close(eng, oracle, dtype):
    """every gradient sum against oracle.G under the arithmetic's rule; returns the largest relative Frobenius error"""
    got = engine_grads(eng)
    worst = max([_rel_fro(got[k], w) for k, w in oracle.G.items() if w.any() and not _dead_bias(oracle, k)] + [0.0])
    if dtype != "bfloat16":
        _check_grads(eng, oracle)
        return worst
    for k, want in oracle.G.items():
        if _dead_bias(oracle, k):
            continue
        if not want.any():
            assert np.abs(got[k]).max() <= 2e-5 * 1e-3, k
        else:
            assert _rel_fro(got[k], want) <= 2e-3, (k, _rel_fro(got[k], want))
    return worst


# ================= A. softmax cross-entropy, the training pass =================

NET_A = dict(input_dim=20, num_layers=1, num_units=32, nonlin="tanh", batch_norm=False, init_learning_rate=1e-3, num_steps=50,
             max_frames=256)
T_A = 19
WIDTHS = [3, 1021, 1024, 1025, 2048, 2049, 4094, 4097, 8192, 8193]
XENT_CASES = [("float32", O) for O in WIDTHS] + [(d, O) for d in ("float32_mfma", "bfloat16") for O in (1025, 4097, 8193)]


def _width(O):
    """(float4 per thread of the kernel the dispatch picks, 0 = generic; live columns of the last float4)"""
    nc4 = (O + 3) // 4
    return next((nv for nv in (1, 2, 4, 8) if nc4 <= 256 * nv), 0), O - 4 * ((O - 1) // 4)


def _forced_labels(rng, T, O):
    """column 0, column O - 1, one label in every slot of the last live float4, the rest random"""
    y = rng.integers(0, O, size=T)
    y[0], y[1] = 0, O - 1
    for i, c in enumerate(range(4 * ((O - 1) // 4), O)):
        y[2 + i] = c
    return y.astype(np.int32)


def _xent64(z, y):
    """float64 (loss per row, softmax - onehot) of the fp32 logits z"""
    z = np.asarray(z, dtype=np.float64)
    mx = z.max(axis=1, keepdims=True)
    ex = np.exp(z - mx)
    se = ex.sum(axis=1, keepdims=True)
    rows = np.arange(len(y))
    loss = (mx + np.log(se))[:, 0] - z[rows, y]
    grad = ex / se
    grad[rows, y] -= 1.0
    return loss, grad


def _eval_pass(eng, X, y):
    from tfkaldi_amd import _lib
    eng.zero_accumulators()
    eng.eval_accumulate(X, y)
    return eng.debug_fetch(_lib.DBG_LOGITS, 0, len(y)), eng.scalar(_lib.BATCH_LOSS)


@pytest.mark.parametrize("regime", ["initial", "peaked"])
@pytest.mark.parametrize("dtype,O", XENT_CASES, ids=["%s-%d" % c for c in XENT_CASES])
def test_softmax_xent_every_width(nets, dtype, O, regime):
    from tfkaldi_amd import _lib
    kw = dict(NET_A, output_dim=O)
    eng = nets(dtype, **kw)
    rng = np.random.default_rng(100 + O)
    oracle = _oracle(kw, dtype, rng)
    copy_oracle_to_engine(oracle, eng)
    X = batch(rng, T_A, kw["input_dim"], O)[0]
    y = _forced_labels(rng, T_A, O)
    under_rows = np.arange(6, 9)
    if regime == "peaked":
        z0, _ = _eval_pass(eng, X, y)
        factor = np.float32(140.0 / (z0.max(axis=1) - z0.min(axis=1)).min())
        for p in (oracle.W, oracle.b):
            p[oracle.L] = (p[oracle.L].astype(np.float32) * factor).astype(np.float64)
        copy_oracle_to_engine(oracle, eng)
        z1, _ = _eval_pass(eng, X, y)
        y[under_rows] = z1[under_rows].argmin(axis=1)  # labels on the smallest logit of their row
    zdev, eval_loss = _eval_pass(eng, X, y)
    want_rows, want_grad = _xent64(zdev, y)
    want_loss = float(want_rows.sum())
    spread = float((zdev.max(axis=1) - zdev.min(axis=1)).min())
    if regime == "peaked":
        assert (zdev == z1).all() and spread > 110, spread
        assert np.isfinite(want_rows).all() and (want_rows[under_rows] > 100).all(), want_rows[under_rows]
    nv, tail = _width(O)
    head = "dnn-edges A xent %-12s O %4d NV %d tail %d %-7s spread %7.1f |" % (dtype, O, nv, tail, regime, spread)
    if _rel(eval_loss, want_loss) > 2e-5:  # (print the figure before the assertion stops the case)
        print("%s device: eval loss %.1e" % (head, _rel(eval_loss, want_loss)))
    assert_close("eval loss", eval_loss, want_loss, 2e-5, 0)
    eng.zero_accumulators()
    eng.accumulate(X, y)
    loss, dlog = eng.scalar(_lib.BATCH_LOSS), eng.debug_fetch(_lib.DBG_LOGITS, 0, T_A)
    oracle.forward_logits(X)
    oracle.backward_from_dlogits(want_grad, want_loss, T_A)
    got = engine_grads(eng)
    print("%s device: eval loss %.1e loss %.1e dlogits %.1e | gradients fro %s" % (
        head, _rel(eval_loss, want_loss), _rel(loss, want_loss), np.abs(dlog - want_grad).max(),
        " ".join("%s %.1e" % (k, _rel_fro(got[k], oracle.G[k])) for k in sorted(got))))
    assert eng.scalar(_lib.NUM_FRAMES) == T_A
    assert_close("training loss against the evaluation pass's", loss, eval_loss, 1e-6, 0)
    assert_close("loss", loss, want_loss, 2e-5, 0)
    assert_close("dlogits", dlog, want_grad, rtol=1e-4, atol=2e-6)
    if regime == "peaked":
        # expf(z - max) is 0 in fp32 below -103.98 (half the smallest denormal): there dLogits is 0 * (1 / sum) - onehot
        under = (zdev - zdev.max(axis=1, keepdims=True)) < -104.5
        label = np.zeros_like(under)
        label[np.arange(T_A), y] = True
        assert under[under_rows, y[under_rows]].all() and (under & ~label).any()
        assert (dlog[under & label] == -1.0).all()
        rest = dlog[under & ~label]
        assert (rest == 0.0).all() and not np.signbit(rest).any()
    _grads_close(eng, oracle, dtype)


def test_softmax_xent_stacked_padding_rows(nets):
    """accumulate_stacked with rows [100, 37] at O = 4097 (NV = 8, tail 1): 128 + 128 rows in the pass, 119 of them padding whose
    label is -1 -- loss 0, a zero gradient row in dLogits and in its twin (the output layer's dW reads the twin over ALL rows)"""
    from tfkaldi_amd import _lib
    O, rows = 4097, [100, 37]
    kw = dict(NET_A, output_dim=O, nonlin="relu", batch_norm=True)
    eng, seq = nets("float32", **kw), _engine(kw, "float32")
    rng = np.random.default_rng(4097)
    oracle = _oracle(kw, "float32", rng)
    for e in (eng, seq):
        copy_oracle_to_engine(oracle, e)
    parts = [(batch(rng, n, kw["input_dim"], O)[0], _forced_labels(rng, n, O)) for n in rows]
    X, y = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    eng.zero_accumulators()
    eng.accumulate_stacked(X, y, rows)
    span = 128  # rows per segment in the pass (engine.hip: stack_align of the emulated arithmetic)
    dlog = eng.debug_fetch(_lib.DBG_LOGITS, 0, span * len(rows))
    worst = 0.0
    seq.zero_accumulators()
    for i, (Xs, ys) in enumerate(parts):
        seq.accumulate(Xs, ys)
        oracle.accumulate(Xs, ys)
        want = _xent64(oracle.last_logits, ys)[1]
        seg = dlog[i * span:i * span + rows[i]]
        worst = max(worst, np.abs(seg - want).max())
        assert_close("dlogits of segment %d" % i, seg, want, rtol=1e-4, atol=2e-6)
        assert not dlog[i * span + rows[i]:(i + 1) * span].any(), "padding rows of segment %d" % i
    g_stk, g_seq = engine_grads(eng), engine_grads(seq)
    l_stk, l_seq = eng.scalar(_lib.BATCH_LOSS), seq.scalar(_lib.BATCH_LOSS)
    print("dnn-edges A xent stacked %s O %d | device: loss %.1e (sequential %.1e) dlogits %.1e | gradients fro %s" % (
        rows, O, _rel(l_stk, oracle.batch_loss), _rel(l_stk, l_seq), worst,
        " ".join("%s %.1e" % (k, _rel_fro(g_stk[k], oracle.G[k])) for k in sorted(g_stk) if not _dead_bias(oracle, k))))
    assert eng.scalar(_lib.NUM_FRAMES) == seq.scalar(_lib.NUM_FRAMES) == sum(rows)
    for k in g_seq:  # the bounds of tests/test_gpu_stacked.py at its first step
        layer = "".join(ch for ch in k if ch.isdigit())
        scale = max(np.abs(v).max() for kk, v in g_seq.items() if kk.endswith(layer)) + 1e-30
        assert np.abs(g_stk[k] - g_seq[k]).max() <= 2e-6 * scale, (k, np.abs(g_stk[k] - g_seq[k]).max() / scale)
    assert abs(l_stk - l_seq) <= 2e-6 * abs(l_seq)
    assert_close("loss", l_stk, oracle.batch_loss, 2e-5, 0)
    _check_grads(eng, oracle)
    seq.close()


# ================= B. batch-norm statistics =================

NET_B = dict(input_dim=20, num_layers=2, num_units=130, output_dim=13, batch_norm=True, init_learning_rate=1e-3, num_steps=50,
             max_frames=4225)
CHAINS = {"relu": dict(nonlin="relu"), "tanh-l2": dict(nonlin="tanh", l2_norm=True), "relu-drop": dict(nonlin="relu", keep_prob=0.7)}
ROWS_B = [1, 2, 3, 31, 33, 63, 64, 65, 127, 128, 129, 257, 1025, 1089, 2049, 2113, 2177, 4097, 4225]
ROWS_OTHER = [1, 65, 129, 1089, 2177, 4225]
BN_CASES = ([("float32", c, T) for c in ("relu", "tanh-l2") for T in ROWS_B] + [("float32", "relu-drop", T) for T in (65, 2177, 4225)]
            + [(d, c, T) for d in ("float32_mfma", "bfloat16") for c in ("relu", "tanh-l2") for T in ROWS_OTHER])
# every case on ordinary data and, from two rows on, on offset data (one row has no spread to offset: every variance is 0)
BN_CASES = [c + (v,) for c in BN_CASES for v in ("ordinary", "offset") if v == "ordinary" or c[2] >= 2]


def _model_chunks(dtype, chain, T):
    """rows per chunk of the device's per-chunk statistics"""
    if chain == "tanh-l2":  # bn_stats_train: blocks of 32 rows, at most kMaxRowSplits = 256 of them
        rs = min((T + 31) // 32, 256)
        return [(T + rs - 1) // rs]
    return [128] if dtype == "float32" else [64, 128]


def _within(name, got, want, tol):
    err = np.abs(got.astype(np.float64) - want)
    if not (err <= tol).all():
        c = int(np.argmax(err / tol))
        raise AssertionError("%s: |%.9g - %.9g| = %.3g > %.3g in column %d (%d of %d columns)" % (
            name, got[c], want[c], err[c], tol[c], c, int((err > tol).sum()), err.size))


@pytest.mark.parametrize("dtype,chain,T,variant", BN_CASES, ids=["%s-%s-%d-%s" % c for c in BN_CASES])
def test_batch_norm_statistics(nets, dtype, chain, T, variant):
    from tfkaldi_amd import _lib
    kw = dict(NET_B, **CHAINS[chain])
    eng = nets(dtype, **kw)
    L, H, F, keep = kw["num_layers"], kw["num_units"], kw["input_dim"], kw.get("keep_prob", 1.0)
    rng = np.random.default_rng(1000 * T + len(chain))
    oracle = _oracle(kw, dtype, rng)
    if variant == "offset":
        W, b = offset_layer(rng, F, H, 1.5, CONSTANT_COL)
        oracle.W[0], oracle.b[0] = W.astype(np.float64), b.astype(np.float64)
        oracle.beta[0][CONSTANT_COL] = 0.25  # (positive: a ReLU must not hide what the column's output is)
    copy_oracle_to_engine(oracle, eng)
    mov0 = [(oracle.mov_mean[l].copy(), oracle.mov_var[l].copy()) for l in range(L)]
    X, y = batch(rng, T, F, kw["output_dim"])
    eng.zero_accumulators()
    eng.accumulate(X, y)
    masks = [eng.debug_fetch(_lib.DBG_DROPOUT_MASK, l, T).astype(np.float64) for l in range(L)] if keep < 1 else None
    hidden, refs, figures, failures = [], [], [], []
    for l in range(L):
        z = eng.debug_fetch(_lib.DBG_PREACT, l, T)
        mean_d, rstd_d = eng.debug_fetch(_lib.DBG_BN_MEAN, l, T)[0], eng.debug_fetch(_lib.DBG_BN_RSTD, l, T)[0]
        hid = eng.debug_fetch(_lib.DBG_HIDDEN, l, T)
        (mean, var, rstd), scale, (e_mean, e_rstd), (tol_mean, tol_rstd) = _stat_bounds(z, _model_chunks(dtype, chain, T))
        v = _nonlin((z.astype(np.float64) - mean) * rstd + oracle.beta[l], kw["nonlin"])
        if kw.get("l2_norm"):
            s = (v ** 2).mean(axis=1, keepdims=True)
            v = np.where(s > 1, v / s, v)
        want_hid = v if masks is None else v * masks[l] / keep
        figures.append((e_mean, float((np.abs(mean_d - mean) / scale).max()), e_rstd, float((np.abs(rstd_d - rstd) / rstd).max()),
                        float(np.abs(hid - want_hid).max())))
        hidden.append(hid)
        refs.append((z, mean, var, rstd, want_hid, mean_d, rstd_d, tol_mean, tol_rstd))
    print("dnn-edges B stats %-12s %-9s T %4d %-8s | %s" % (dtype, chain, T, variant, " | ".join(
        "layer %d mean: model %.1e device %.1e  rstd: model %.1e device %.1e  hidden %.1e" % ((l,) + figures[l]) for l in range(L))))
    for l, (z, mean, var, rstd, want_hid, mean_d, rstd_d, tol_mean, tol_rstd) in enumerate(refs):
        assert np.isfinite(hidden[l]).all()
        _within("mean of layer %d" % l, mean_d, mean, tol_mean)
        _within("rstd of layer %d" % l, rstd_d, rstd, tol_rstd)
        assert_close("hidden%d" % l, hidden[l], want_hid, 1e-4, 2e-5)
        constant = np.arange(H) if T == 1 else np.array([CONSTANT_COL] if (variant == "offset" and l == 0) else [], dtype=int)
        if constant.size:  # variance exactly 0: rstd = 1 / sqrt(eps), the output is nonlin(beta)
            assert not var[constant].any()
            np.testing.assert_allclose(rstd_d[constant], 1 / np.sqrt(BN_EPS), rtol=1e-6)
            if not kw.get("l2_norm") or kw["nonlin"] == "tanh":  # (tanh: the row's mean square stays below 1, L2Norm is the identity)
                flat = _nonlin(oracle.beta[l], kw["nonlin"])[constant] * (1.0 if masks is None else masks[l][:, constant] / keep)
                assert_close("hidden%d of the constant columns" % l, hidden[l][:, constant], np.broadcast_to(flat, (T, constant.size)),
                             1e-4, 2e-5)
    # backward: every gradient against the oracle on the device's own pre-activations
    oracle.zdev = [r[0] for r in refs]
    if kw["nonlin"] == "relu":
        active = [hidden[l] > 0 if masks is None else np.where(masks[l] > 0, hidden[l] > 0, True) for l in range(L)]
        oracle.accumulate(X, y, masks=masks, relu_active=active)
        band, limit = (1e-2, 1e-3) if dtype == "bfloat16" else (1e-4, 1e-4)
        for l, c in enumerate(oracle.last_cache):
            dis = c["own_active"] != active[l]
            if masks is not None:
                dis &= masks[l] > 0
            assert dis.sum() <= max(1, limit * dis.size), (l, int(dis.sum()), dis.size)
            if dis.any():
                assert np.abs(c["u"][dis]).max() < band, (l, np.abs(c["u"][dis]).max())
    else:
        oracle.accumulate(X, y, masks=masks)
    loss = eng.scalar(_lib.BATCH_LOSS)
    assert eng.scalar(_lib.NUM_FRAMES) == T
    assert_close("batch_loss", loss, oracle.batch_loss, 5e-4 if dtype == "bfloat16" else 2e-5, 0)
    worst = _grads_close(eng, oracle, dtype)
    if T == 1:  # one row: dz = rstd * (du - mean(du) - xhat * mean(du * xhat)) is 0, so is everything below the batch norms
        assert not any(oracle.G["W%d" % l].any() for l in range(L))
    print("dnn-edges B grads %-12s %-9s T %4d %-8s | loss %.1e gradients fro %.1e" % (dtype, chain, T, variant,
                                                                                      _rel(loss, oracle.batch_loss), worst))
    assert_close("avg loss", eng.apply(), oracle.apply(), 5e-4 if dtype == "bfloat16" else 2e-5, 0)
    d = oracle.bn_decay
    for l, (z, mean, var, rstd, _, _, _, _, _) in enumerate(refs):  # moving averages from the float64 statistics of zdev
        assert_close("mov_mean%d" % l, eng.get(_lib.BN_MOVING_MEAN, l), d * mov0[l][0] + (1 - d) * mean, 1e-5, 1e-6)
        assert_close("mov_var%d" % l, eng.get(_lib.BN_MOVING_VAR, l), d * mov0[l][1] + (1 - d) * var, 1e-5, 1e-6)


# ================= C. Adam =================

SMALL = dict(input_dim=22, num_layers=2, num_units=36, output_dim=13, nonlin="relu", init_learning_rate=1e-3, num_steps=100,
             max_frames=256)
T_C = 20


def _adam_values(T):
    """G / T: zero and signed zero, the clip boundary and its fp32 neighbours, squares that underflow to a denormal (1e-40) and to
    zero (1e-60), the largest finite gradient sum"""
    f = np.float32
    below, above = float(np.nextafter(f(1), f(0))), float(np.nextafter(f(1), f(2)))
    mags = [1.0, below, above, 1e-4, 1e-20, 1e-30, 3e38 / T]
    return np.array([0.0, -0.0] + [s * m for m in mags for s in (1.0, -1.0)], dtype=np.float64)


@pytest.mark.parametrize("dtype,units", [("float32", 36), ("bfloat16", 36), ("bfloat16", 40)])
def test_adam_on_the_values_where_it_can_go_wrong(gpu, dtype, units):
    """test_adam_known_answer's harness (gradient sums injected through SLOT_GRAD after a T-frame accumulate, 3 steps) with the
    edge values tiled over every tensor, the tile moved on by 5 per step and by 3 per tensor so that an element's moments see
    different values.  40 units: every leading dimension a multiple of 8, where mixed precision keeps a bf16 shadow that mirrors
    the weight arena and adam_kernel writes it with the update (36 units: the shadow is rebuilt from the parameters)."""
    from tfkaldi_amd import _lib
    rng = np.random.default_rng(3)
    kw = dict(SMALL, num_units=units)
    eng, mirror = _engine(kw, dtype), _engine(kw, dtype)
    # (the oracle takes the fp32 values of the hyperparameters the kernel is given: 1 - float32(0.999) is 1.3e-5 off 1e-3)
    oracle = _oracle(kw, dtype, rng, beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)),
                     adam_epsilon=float(np.float32(1e-8)))
    copy_oracle_to_engine(oracle, eng)
    X, y = batch(rng, T_C, kw["input_dim"], kw["output_dim"])
    eng.accumulate(X, y)
    oracle.accumulate(X, y)
    vals = (_adam_values(T_C) * T_C).astype(np.float32)
    assert np.isfinite(vals).all() and np.signbit(vals[1]) and vals[1] == 0
    weights = sorted(eng.buckets()[:eng.L + 1])
    w0, w_end = weights[0][0], weights[-1][0] + weights[-1][1]
    checked = "logits"
    for step in range(3):
        n = 0
        for l in range(eng.L + 1):
            for kind, name in ((_lib.WEIGHTS, "W%d" % l), (_lib.BIASES, "b%d" % l)):
                g = np.resize(np.roll(vals, 5 * step + 3 * n), oracle.G[name].shape)
                eng.set(kind, l, g, _lib.SLOT_GRAD)
                oracle.G[name] = g.astype(np.float64)
                n += 1
        eng.apply()
        oracle.apply()
        got, errs = engine_params(eng), [0.0, 0.0, 0.0]
        for l in range(eng.L + 1):
            for kind, k in ((_lib.WEIGHTS, "W%d" % l), (_lib.BIASES, "b%d" % l)):
                m, v = eng.get(kind, l, _lib.SLOT_ADAM_M), eng.get(kind, l, _lib.SLOT_ADAM_V)
                errs = [max(e, float(np.abs(a - b).max())) for e, a, b in zip(errs, (got[k], m, v), (oracle.params()[k], oracle.m[k],
                                                                                                     oracle.v[k]))]
                assert_close("%s step %d" % (k, step), got[k], oracle.params()[k], 1e-5, 2e-6)
                assert_close("m[%s] step %d" % (k, step), m, oracle.m[k], 1e-5, 1e-38)  # (atol: the smallest normal fp32)
                assert_close("v[%s] step %d" % (k, step), v, oracle.v[k], 1e-5, 1e-12)
        assert all((g == 0).all() for g in engine_grads(eng).values())
        # the operand twins the optimiser wrote with the update against twins rebuilt from the parameters: through what the
        # contractions compute from them (`mirror` builds a fresh set from the same parameters) ...
        for k, p in got.items():
            mirror.set(_lib.WEIGHTS if k.startswith("W") else _lib.BIASES, int(k[1:]), p)
        np.testing.assert_allclose(eng.posteriors(X, raw_logits=True), mirror.posteriors(X, raw_logits=True), rtol=1e-6, atol=0)
        # ... and, where the optimiser writes them itself, bit for bit
        if dtype == "float32":
            before = eng.param_checksum(3)
            assert eng.twins_from_params(w0, w_end - w0) is True
            assert eng.param_checksum(3) == before, "three-plane twins written by adam_kernel, step %d" % step
            checked = "logits + checksum of the three-plane twins"
        elif units % 8 == 0:
            before = eng.param_checksum(1)
            eng.params_touched()
            eng.posteriors(X, raw_logits=True)  # (the forward pass rebuilds a shadow that is not current)
            assert eng.param_checksum(1) == before, "bf16 shadow written by adam_kernel, step %d" % step
            checked = "logits + checksum of the bf16 shadow"
        print("dnn-edges C adam %-9s H %d step %d | device: parameters %.1e m %.1e v %.1e | twins: %s" % (
            (dtype, units, step) + tuple(errs) + (checked,)))
        if step < 2:
            eng.accumulate(X, y)
            oracle.accumulate(X, y)
    eng.close(); mirror.close()
