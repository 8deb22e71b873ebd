"""CPU ORACLE (test infrastructure, NOT product code) for the DNN training hot path of vrenkens/tfkaldi.

A float64 numpy restatement of what the reference's TensorFlow graph computes for
neuralNetworks/trainer.py (Trainer / CrossEnthropyTrainer), neuralNetworks/decoder.py (Decoder) and
neuralNetworks/classifiers/{dnn,layer,activation,seq_convertors}.py.  Only tests/, __graft_entry__.smoke()
and bench.py's cpu_baseline leg may import this package; the product (tfkaldi_amd/) never does.

PARITY PINNING.  The arithmetic of this path lives in TensorFlow (import at trainer.py:5, nnet.py:8,
decoder.py:3, classifiers/*.py), a third-party dependency that is absent from /root/reference, not
pinned by it (no requirements file; README.md:12 points at TF 0.6, the API used bounds it to ~0.10-0.12)
and not installable here; the reference holds no tests, golden vectors or fixtures for the path
(SURVEY.md section 4, 8c).  The TensorFlow half of this oracle is therefore **parity unpinned**: it
restates the published TF-0.1x semantics of the ops at the reference's call sites, flagged ASSUMPTION
below where the behaviour is not visible in the reference tree, and is cross-checked against PyTorch
autograd (tests/test_oracle.py) and the known-answer properties of SURVEY.md section 8c.  The numpy
half of the reference (processing/*.py) IS importable; its golden vectors are in tests/golden/ (made by
oracle/make_golden_io.py).

ASSUMPTIONS (TF-0.1x behaviour outside the reference tree):
  A1 tf.contrib.layers.batch_norm defaults: decay 0.999, epsilon 1e-3, center (beta) only, no gamma,
     batch variance biased (tf.nn.moments), moving_mean init 0 / moving_variance init 1, the moving
     variance tracks the biased batch variance, one EMA update per session.run of the training graph.
  A2 tf.train.AdamOptimizer defaults beta1 .9, beta2 .999, epsilon 1e-8;
     lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t); w -= lr_t * m / (sqrt(v) + epsilon); t starts at 1.
  A3 tf.train.exponential_decay non-staircase: lr = init * decay ** (global_step / num_steps).
  A4 tf.nn.dropout(x, keep) = x / keep * Bernoulli(keep) mask.
  A5 tf.nn.softmax_cross_entropy_with_logits = logsumexp(z) - z[y] for one-hot labels.
"""
import numpy as np

NONLINS = ("relu", "sigmoid", "tanh", "linear")


def _nonlin(u, kind):
    """activation.py:84 applied with the function chosen at nnet.py:48-62."""
    if kind == "relu":
        return np.maximum(u, 0.0)
    if kind == "sigmoid":
        return 1.0 / (1.0 + np.exp(-u))
    if kind == "tanh":
        return np.tanh(u)
    if kind == "linear":
        return u
    raise Exception('unkown nonlinearity')  # nnet.py:65


def _nonlin_grad(v, kind):
    """derivative of the nonlinearity expressed through its output v."""
    if kind == "relu":
        return (v > 0).astype(np.float64)
    if kind == "sigmoid":
        return v * (1.0 - v)
    if kind == "tanh":
        return 1.0 - v * v
    return np.ones_like(v)


def round_bf16(x):
    """float -> nearest bfloat16 (ties to even), returned as float64; as the engine rounds its fp32 values"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


class OracleDNN(object):
    """State + ops of Trainer (trainer.py:13-218) around DNN (dnn.py:10-131), in float64."""

    def __init__(self, input_dim, num_layers, num_units, output_dim, nonlin="relu", batch_norm=False,
                 l2_norm=False, keep_prob=1.0, layerwise_init=False, init_learning_rate=1e-3,
                 learning_rate_decay=1.0, num_steps=1, bn_decay=0.999, bn_epsilon=1e-3, beta1=0.9, beta2=0.999,
                 adam_epsilon=1e-8, gemm_dtype="float32"):
        assert nonlin in NONLINS
        # "bfloat16": restates the engine's mixed-precision mode (TFK_DTYPE_BF16, not a reference behaviour): the
        # operands of the three contractions are rounded to bfloat16, everything else keeps full precision
        assert gemm_dtype in ("float32", "bfloat16")
        self.gemm_dtype = gemm_dtype
        assert 0 < keep_prob  # activation.py:126 (values > 1 never reach Dropout: nnet.py:70-72)
        self.F, self.L, self.H, self.O = input_dim, num_layers, num_units, output_dim
        self.nonlin, self.bn, self.l2 = nonlin, bool(batch_norm), bool(l2_norm)
        self.keep = float(keep_prob)
        self.dropout = self.keep < 1  # nnet.py:70
        self.layerwise = bool(layerwise_init)
        self.init_lr, self.decay, self.num_steps = init_learning_rate, learning_rate_decay, num_steps
        self.bn_decay, self.bn_eps = bn_decay, bn_epsilon
        self.b1, self.b2, self.eps = beta1, beta2, adam_epsilon
        dims = [input_dim] + [num_units] * num_layers + [output_dim]
        # layer.py:42-48: weights [d_in, d_out], biases zeros.  Hidden weights are injected by the caller
        # (random init cannot match TF); dnn.py:67-68 + layer.py:39-44: output weights stddev 0 => zeros.
        self.W = [np.zeros((dims[l], dims[l + 1])) for l in range(num_layers + 1)]
        self.b = [np.zeros(dims[l + 1]) for l in range(num_layers + 1)]
        self.beta = [np.zeros(num_units) for _ in range(num_layers)]       # A1: center=True
        self.mov_mean = [np.zeros(num_units) for _ in range(num_layers)]   # A1
        self.mov_var = [np.ones(num_units) for _ in range(num_layers)]     # A1
        self.global_step = 0        # trainer.py:98-100
        self.lr_fact = 1.0          # trainer.py:104-106
        self.initialisedlayers = 0  # dnn.py:85-89
        self.adam_t = 0             # Adam's beta-power step count (A2)
        self._zero_accumulators()
        self.m = self._like_params()
        self.v = self._like_params()

    def _mm(self, a, b):
        """a . b in the arithmetic of the contractions"""
        if self.gemm_dtype == "bfloat16":
            return round_bf16(a).dot(round_bf16(b))
        return a.dot(b)

    # ---- parameter bookkeeping ----
    def params(self):
        """tf.trainable_variables() of the classifier (trainer.py:82): W, b of every layer, BN beta."""
        p = {}
        for l in range(self.L + 1):
            p["W%d" % l] = self.W[l]
            p["b%d" % l] = self.b[l]
        if self.bn:
            for l in range(self.L):
                p["beta%d" % l] = self.beta[l]
        return p

    def _like_params(self):
        return {k: np.zeros_like(v) for k, v in self.params().items()}

    def _zero_accumulators(self):
        self.G = self._like_params()   # trainer.py:118-122, init_grads :350
        self.batch_loss = 0.0          # trainer.py:91-93,  init_loss :351
        self.num_frames = 0            # trainer.py:126-128, init_num_frames :352

    def init_hidden_weights(self, rng):
        """layer.py:39-44: N(0, 1/sqrt(d_in)) for the hidden layers; returns the float32 values used."""
        out = []
        for l in range(self.L):
            d_in = self.W[l].shape[0]
            w = (rng.standard_normal(self.W[l].shape) / np.sqrt(d_in)).astype(np.float32)
            self.W[l] = w.astype(np.float64)
            out.append(w)
        return out

    def num_active(self):
        """dnn.py:97-102: tf.case selects activations[initialisedlayers], default activations[-1]."""
        if not self.layerwise:
            return self.L
        n = self.initialisedlayers + 1
        return self.L if (n > self.L or self.initialisedlayers < 0) else n

    def learning_rate(self):
        """trainer.py:110-112 (A3)."""
        return self.init_lr * self.decay ** (float(self.global_step) / self.num_steps) * self.lr_fact

    # ---- forward ----
    def _forward(self, X, train, masks=None, nfw=None, relu_active=None):
        """dnn.py:73-108 on flat frames X[T, F] (seq2nonseq, seq_convertors.py:12-39, is the caller's
        utterance-major concatenation).  Returns logits and the per-layer cache for backward.

        relu_active (test hook, ReLU nets only): per hidden layer a boolean [T, H] on/off pattern that REPLACES the
        oracle's own `u > 0` in the forward pass and in the derivative.  A unit whose pre-activation lies within
        fp32 round-off of the kink can come out on the other side in an fp32 implementation; pinning the pattern to
        the one the implementation chose lets every gradient be compared element-wise, while the caller asserts
        how rare (and how close to the kink) the disagreements are."""
        nact = self.num_active()
        if nfw is None:
            nfw = nact
        cache = []
        inp = np.asarray(X, dtype=np.float64)
        T = inp.shape[0]
        for l in range(nfw):
            c = {"in": inp}
            z = self._mm(inp, self.W[l]) + self.b[l]                 # layer.py:52
            u = z
            if self.bn:                                               # activation.py:159-161 (A1)
                if train:
                    mu = z.mean(axis=0)
                    var = ((z - mu) ** 2).mean(axis=0)                # biased
                    c["batch_mean"], c["batch_var"] = mu, var
                else:
                    mu, var = self.mov_mean[l], self.mov_var[l]
                rstd = 1.0 / np.sqrt(var + self.bn_eps)
                xhat = (z - mu) * rstd
                u = xhat + self.beta[l]
                c["xhat"], c["rstd"] = xhat, rstd
            v = _nonlin(u, self.nonlin)                               # activation.py:84
            if relu_active is not None:
                assert self.nonlin == "relu"
                c["own_active"], c["u"] = u > 0, u
                c["dact"] = np.asarray(relu_active[l], dtype=np.float64)
                v = u * c["dact"]
            c["v"] = v
            w = v
            if self.l2:                                               # activation.py:101-111
                s = (v ** 2).mean(axis=1, keepdims=True)              # the mean SQUARE, not its root
                w = np.where(s > 1, v / s, v)
                c["s"] = s
            a = w
            if self.dropout and train:                                # activation.py:140-141 (A4)
                mask = masks[l]
                a = w * mask / self.keep
                c["mask"] = mask
            c["a"] = a
            cache.append(c)
            inp = a
        logits = self._mm(cache[nact - 1]["a"], self.W[self.L]) + self.b[self.L]  # dnn.py:108, identity activation
        return logits, cache, nact

    @staticmethod
    def _xent(logits, y):
        """trainer.py:526-531 (A5): summed softmax cross-entropy and softmax probabilities."""
        mx = logits.max(axis=1, keepdims=True)
        ex = np.exp(logits - mx)
        se = ex.sum(axis=1, keepdims=True)
        lse = (mx + np.log(se))[:, 0]
        loss = float((lse - logits[np.arange(len(y)), y]).sum())
        return loss, ex / se

    # ---- update_gradients_op: one micro-batch (trainer.py:160-169) ----
    def accumulate(self, X, y, masks=None, relu_active=None):
        """Forward (train) + loss + backward; G += g, batch_loss += loss, num_frames += T, BN EMA.
        masks: per hidden layer 0/1 keep masks [T, H] when dropout is on.  relu_active: see _forward.  Returns the
        dict of this micro-batch's gradients (tf.gradients, trainer.py:155) for inspection."""
        y = np.asarray(y).astype(np.int64)
        T = len(y)
        logits, cache, nact = self._train_forward(X, masks, relu_active)
        loss, prob = self._xent(logits, y)
        dz = prob.copy()
        dz[np.arange(T), y] -= 1.0                                    # d(sum CE)/dlogits
        return self._backward_and_accumulate(dz, loss, T, logits, cache, nact)

    def _train_forward(self, X, masks=None, relu_active=None):
        # All BN layers' UPDATE_OPS are fetched (trainer.py:164-169), so with layer-wise growth the
        # hidden layers above the active depth are still evaluated in training mode.
        nfw = self.L if (self.layerwise and self.bn) else None
        return self._forward(X, True, masks, nfw, relu_active)

    # Loss-agnostic entry points (used with the CTC oracle, oracle/ctc_oracle.py): the training-mode logits of a
    # micro-batch, then the rest of update_gradients_op from a given d loss / d logits.
    def forward_logits(self, X, train=True, masks=None):
        if not train:
            return self._forward(X, False)[0]
        self._pending = self._train_forward(X, masks)
        return self._pending[0]

    def backward_from_dlogits(self, dlogits, loss, num_frames):
        logits, cache, nact = self._pending
        return self._backward_and_accumulate(np.asarray(dlogits, dtype=np.float64), loss, num_frames, logits, cache, nact)

    def _backward_and_accumulate(self, dz, loss, num_frames, logits, cache, nact):
        g = self._like_params()
        g["W%d" % self.L] = self._mm(cache[nact - 1]["a"].T, dz)
        g["b%d" % self.L] = dz.sum(axis=0)
        da = self._mm(dz, self.W[self.L].T)
        for l in range(nact - 1, -1, -1):
            c = cache[l]
            dw = da
            if self.dropout:
                dw = da * c["mask"] / self.keep
            dv = dw
            if self.l2:
                s, v = c["s"], c["v"]
                dot = (dw * v).sum(axis=1, keepdims=True)
                dv = np.where(s > 1, dw / s - v * (2.0 * dot / (self.H * s * s)), dw)
            du = dv * (c["dact"] if "dact" in c else _nonlin_grad(c["v"], self.nonlin))
            if self.bn:
                g["beta%d" % l] = du.sum(axis=0)
                xhat, rstd = c["xhat"], c["rstd"]
                dzl = rstd * (du - du.mean(axis=0) - xhat * (du * xhat).mean(axis=0))
            else:
                dzl = du
            g["W%d" % l] = self._mm(c["in"].T, dzl)
            g["b%d" % l] = dzl.sum(axis=0)
            if l > 0:
                da = self._mm(dzl, self.W[l].T)
        for k in g:                                                   # trainer.py:165-169
            self.G[k] = self.G[k] + g[k]
        self.batch_loss += loss
        self.num_frames += num_frames
        if self.bn:                                                   # UPDATE_OPS (A1)
            for l in range(len(cache)):
                d = self.bn_decay
                self.mov_mean[l] = d * self.mov_mean[l] + (1 - d) * cache[l]["batch_mean"]
                self.mov_var[l] = d * self.mov_var[l] + (1 - d) * cache[l]["batch_var"]
        self.last_logits, self.last_cache = logits, cache
        return g

    # ---- [average_loss, apply_gradients_op] + re-initialisation (trainer.py:336-352) ----
    def apply(self):
        """mean (trainer.py:174-175) -> clip (:178-179) -> Adam (:182-184, A2); returns the average loss
        evaluated in the same run (pre-update, train mode)."""
        avg_loss = self.batch_loss / float(self.num_frames)          # trainer.py:198
        lr = self.learning_rate()
        self.adam_t += 1
        t = self.adam_t
        lr_t = lr * np.sqrt(1.0 - self.b2 ** t) / (1.0 - self.b1 ** t)
        p = self.params()
        for k in p:
            gk = np.clip(self.G[k] / float(self.num_frames), -1.0, 1.0)
            self.m[k] = self.b1 * self.m[k] + (1 - self.b1) * gk
            self.v[k] = self.b2 * self.v[k] + (1 - self.b2) * gk * gk
            p[k] -= lr_t * self.m[k] / (np.sqrt(self.v[k]) + self.eps)
        self.global_step += 1
        self._zero_accumulators()
        return avg_loss

    # ---- update_valid_loss / average_loss (trainer.py:188-198, 433-441) ----
    def eval_accumulate(self, X, y):
        y = np.asarray(y).astype(np.int64)
        logits, _, _ = self._forward(X, False)
        loss, _ = self._xent(logits, y)
        self.batch_loss += loss
        self.num_frames += len(y)
        self.last_logits = logits

    def eval_finish(self):
        avg = self.batch_loss / float(self.num_frames)
        self.batch_loss, self.num_frames = 0.0, 0
        return avg

    # ---- Decoder (decoder.py:36-44) ----
    def posteriors(self, X):
        logits, _, _ = self._forward(X, False)
        mx = logits.max(axis=1, keepdims=True)
        ex = np.exp(logits - mx)
        return ex / ex.sum(axis=1, keepdims=True)

    # ---- control ops ----
    def halve_learning_rate(self):
        self.lr_fact /= 2.0                                           # trainer.py:141-142

    def add_layer(self):
        self.initialisedlayers += 1                                   # dnn.py:92

    def init_last_layer(self):
        self.W[self.L][...] = 0.0                                     # dnn.py:114-120 (stddev 0, zeros)
        self.b[self.L][...] = 0.0


def reference_microbatches(num_utt, per_minibatch):
    """Index lists of the micro-batches Trainer.update feeds (trainer.py:280-332), including its padding
    quirk: it appends `num_utt % U` zero-length dummies (not U - num_utt % U) and then runs
    floor(len / U) micro-batches.  Returns a list of lists of real utterance indices."""
    U = per_minibatch
    total = num_utt + (num_utt % U)
    out = []
    for k in range(total // U):
        idx = [i for i in range(k * U, (k + 1) * U) if i < num_utt]
        out.append(idx)
    return out


# ---- fp32 reference MODEL of the batch-norm statistics (tests/test_bn_stats_model.py states what it is for) ----
BN_EPS = float(np.float32(1e-3))  # the fp32 value the kernels add to the variance


def stats64(z):
    """float64 column mean, biased variance and rstd of the fp32 matrix z"""
    z = np.asarray(z, dtype=np.float64)
    mean = z.mean(axis=0)
    var = ((z - mean) ** 2).mean(axis=0)
    return mean, var, 1.0 / np.sqrt(var + BN_EPS)


def _running_sum(x):
    return np.add.accumulate(x, axis=0, dtype=np.float32)[-1]  # one fp32 accumulator per column, row after row


def bn_stats_model(z, chunk_rows):
    """fp32 (mean, biased variance, rstd) of the columns of z[T, H]: per chunk of chunk_rows rows a sequential two-pass
    (mean, M2), the chunks merged one after the other (Chan et al.), every operation rounded to float32"""
    z = np.ascontiguousarray(z, dtype=np.float32)
    T = z.shape[0]
    f = np.float32
    n = f(0)
    mean = np.zeros(z.shape[1], dtype=f)
    m2 = np.zeros(z.shape[1], dtype=f)
    for r0 in range(0, T, chunk_rows):
        part = z[r0:r0 + chunk_rows]
        nk = f(part.shape[0])
        mk = _running_sum(part) / nk
        d = part - mk
        qk = _running_sum(d * d)
        tot = n + nk
        delta = mk - mean
        mean = mean + delta * (nk / tot)
        m2 = m2 + qk + delta * delta * (n * nk / tot)
        n = tot
    var = m2 / f(T)
    rstd = f(1) / np.sqrt(var + f(BN_EPS))
    assert mean.dtype == var.dtype == rstd.dtype == f
    return mean, var, rstd


def bn_stat_bounds(z, chunks):
    """The bound tests/test_gpu_dnn_edges.py holds the device's batch mean and rstd to: 4x the error of bn_stats_model against
    float64 on the same z (mean relative to max |z| of its column, rstd relative; the worst column sets the figure; the better
    of the candidate chunk heights), floored at one fp32 ulp of the reference value.  Returns the float64 (mean, var, rstd), the
    columns' scale max |z|, the model's worst errors (e_mean relative to the scale, e_rstd relative) and (tol_mean, tol_rstd)."""
    mean, var, rstd = stats64(z)
    scale = np.maximum(np.abs(z).max(axis=0).astype(np.float64), 1e-30)
    e_mean = e_rstd = np.inf
    for c in chunks:
        m, _, r = bn_stats_model(z, c)
        e_mean = min(e_mean, float((np.abs(m - mean) / scale).max()))
        e_rstd = min(e_rstd, float((np.abs(r - rstd) / rstd).max()))
    tol_mean = np.maximum(4 * e_mean * scale, np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64))
    tol_rstd = np.maximum(4 * e_rstd * rstd, np.spacing(rstd.astype(np.float32)).astype(np.float64))
    return (mean, var, rstd), scale, (e_mean, e_rstd), (tol_mean, tol_rstd)


# ---- the mixed-precision step, link by link on the implementation's OWN operands ----
# A whole-network comparison in bf16 mode cannot be sharp: an operand within fp32 round-off of a bf16 rounding boundary rounds
# the other way in the implementation, moves its frame by ~5e-4, batch norm spreads that to every frame, and one layer later a
# large share of the operands round "at random" (tests/test_bf16_links_host.py shows it on the CPU).  bf16_links is to that
# cascade what relu_active is to the ReLU kink: every link of the chain is restated in float64 on the values the
# implementation itself stored -- the bf16 twins the contractions read, the fp32 tensors everything else reads -- so both sides
# start from bit-identical numbers and each tolerance is an fp32 round-off bound of ONE operation.
GEMM_RTOL, GEMM_ATOL = 4e-7, 1e-6   # fp32 accumulation of exact products: tests/test_gpu_gemm_bf16.py
ACT_RTOL, ACT_ATOL = 1e-4, 2e-5     # a layer output from its pre-activation: tests/test_gpu_dnn_edges.py
SUM_RTOL, SUM_ATOL = 2e-4, 2e-5     # a gradient sum: tests/test_gpu_engine_parity.py (_check_grads)
ULP32 = 2.0 ** -24
LINK_ULPS = 8                       # the "small multiple" of 2^-24 of the element-wise fp32 operations of link B2


def _contract(a, b, add=None):
    """(want, tol) of the fp32-accumulated product of two matrices of bf16 values (+ an fp32 term `add`: a bias or the sum
    accumulated so far): |err| <= 4e-7 * (sum_k |a_k b_k| + |add|) + 1e-6"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    want, mag = a.dot(b), np.abs(a).dot(np.abs(b))
    if add is not None:
        want, mag = want + add, mag + np.abs(add)
    return want, GEMM_RTOL * mag + GEMM_ATOL


def _sum_rule(want):
    return SUM_RTOL * np.abs(want) + SUM_ATOL * max(float(np.abs(want).max()) if want.size else 0.0, 1e-3)


def xent_criterion(y):
    """cross-entropy: dLogits = softmax - onehot of the logits handed in; rtol 1e-4 + atol 2e-6 (tests/test_gpu_engine_parity.py)"""
    y = np.asarray(y).astype(np.int64)

    def crit(logits):
        _, prob = OracleDNN._xent(logits, y)
        prob[np.arange(len(y)), y] -= 1.0
        return prob, 1e-4 * np.abs(prob) + 2e-6
    return crit


def ctc_criterion(utt_len, labels, label_len):
    """the CTC loss: d loss / d logits of oracle/ctc_oracle.py on the logits handed in; rtol 1e-4 + atol 2e-5 below 200 frames,
    2e-4 from there (tests/test_gpu_ctc.py)"""
    def crit(logits):
        from oracle.ctc_oracle import ctc_batch
        _, dlog, _ = ctc_batch(logits, utt_len, labels, label_len, fast=True)
        return dlog, 1e-4 * np.abs(dlog) + (2e-5 if logits.shape[0] < 200 else 2e-4)
    return crit


def bf16_links(net, taps, criterion, stat_chunks=(64, 128), tol_scale=1.0):
    """Every link of one mixed-precision training micro-batch, restated in float64 on the implementation's own operands.

    net       an OracleDNN holding the implementation's fp32 parameters (W, b, beta) and the chain (nonlin, bn, l2, keep)
    taps      what the implementation stored, fp32 tensors and bf16 twins alike as arrays of their exact values:
                X, Xb [T, F];  per evaluated hidden layer z, a, ab [T, H], with batch norm mean, rstd [H], with dropout masks;
                logits (training mode, before the loss), dlogits, dlogb [T, O];  per active layer dzb [T, H] (mixed
                precision stores dz as its twin alone: the kernel rounds it from its registers);
                Wb[l] the weight twins;  G the gradient sums after the micro-batch, G0 those before it (absent: zero);
                nact the active depth (layer-wise growth; absent: all layers).  An "operand" below is always a twin.
    criterion logits -> (want dLogits, tolerance): xent_criterion / ctc_criterion, or the caller's own (MMI)
    Returns (links, got): links a list of (name, want, tol) in float64, got the tapped array of every name.

      F1  z_l = in . W_l + b_l on the operands; the contraction bound 4e-7 * (sum_k |a_k w_k| + |b|) + 1e-6
      F2  mean_l, rstd_l against the float64 statistics of the tapped z_l (bn_stat_bounds)
      F3  a_l against nonlinearity, L2 norm and dropout applied to the tapped z_l, mean_l, rstd_l and beta; rtol 1e-4 + atol 2e-5
      F4  logits = a_{L-1} . W_L + b_L, as F1
      TW  every twin that has an fp32 tensor beside it (Xb, ab_l, dlogb, Wb_l) equals round_bf16 of it, bit for bit (tolerance 0)
      LOSS dLogits against the criterion on the tapped logits
      B1  G[W_l] = G0 + in^T . dz_l on the operands (contraction bound, K = T, |G0| added to the sum); G[b_l] = G0 + the column
          sums of this function's dz_l (the implementation sums its fp32 dz in registers and stores none: the rule plus the
          column sums of B2's fp32 tolerance) and G[beta_l] = G0 + the column sums of this function's du_l, both under the
          gradient-sum rule rtol 2e-4 + atol 2e-5 max |G| (the bias of a batch-normed layer, whose true gradient is zero so that
          max |G| says nothing about the summands: the smaller of _check_grads' rule for it, 1e-4 max(1, max |G[W_l]|), and the
          sum rule plus 8 x 2^-24 x sum |dz|, the round-off of an fp32 sum of T terms in any order up to T = 2^21)
      B2  the twin dzb_l from the operands dz_{l+1}, W_{l+1} and the tapped a_l, z_l, mean_l, rstd_l, masks.  No fp32 dz exists
          to compare the twin with, but rounding to nearest is monotone: an fp32 dz within tol of `want` has its twin in
          [round_bf16(want - tol), round_bf16(want + tol)], tol the fp32 tolerance derived below.  Both ends are the same bf16
          value -- the check is bit for bit -- unless want lies within tol of a rounding boundary, where the two neighbours
          pass; the link is given as that interval's midpoint and half-width.  A truncated twin or one moved to a
          neighbouring value fails it.
      tol_scale multiplies every fp32 tolerance (B2's before the rounding): bf16_links(..., tol_scale=0.25) holds the
      implementation to a quarter of every bound, the head-room check of tests/test_bf16_links_host.py.

    The tolerance of B2, derived (nothing in it is measured on an implementation).  The implementation keeps no du, so the
    link spans the contraction t = dz_{l+1} . W_{l+1}^T and the element-wise chain behind it.
      (1) t carries the contraction bound e_t = 4e-7 * sum_k |dz_k w_k| + 1e-6, element by element.
      (2) du = t * (mask / keep) * act'(v), v the tapped layer output un-scaled (the very fp32 value the implementation takes
          the derivative from, so act' itself differs only by the round-off of evaluating it: relu exact, v (1 - v) and
          1 - v^2 at most 2 ulp of ONE, not of act' -- 1 - v^2 cancels).  |act'| <= 1, so
          e_du = e_t * (mask / keep) * |act'| + LINK_ULPS * 2^-24 * |t| * (mask / keep)
          covers that, the product's two roundings and the scale.  (L2 norm active, s > 1: the row map dv = dw / s - v * 2 (dw .
          v) / (H s^2) is linear in dw; e and the magnitude go through its absolute-value form in the same way.)
      (3) batch norm backward is linear in du: dz = rstd * (du - mean(du) - xhat * mean(du * xhat)).  An error e_du >= 0 on du moves
          dz by at most  rstd * (e_du + mean(e_du) + |xhat| * mean(e_du * |xhat|))  -- the absolute-value form of the map.
      (4) the map's own fp32 evaluation (xhat, two products, an fma, the two column means): every operation is exact to 2^-24 of
          its result and there are fewer than LINK_ULPS of them in a row, so it adds at most
          LINK_ULPS * 2^-24 * rstd * (|du| + mean(|du|) + |xhat| * mean(|du * xhat|)),
          the same absolute-value form applied to the MAGNITUDES; the means are sums of T terms whose partial sums the mean of
          the magnitudes bounds.
      Without batch norm dz = du and the tolerance is e_du."""
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    L, H, keep = net.L, net.H, net.keep
    T = taps["X"].shape[0]
    nfw, nact = len(taps["z"]), taps.get("nact", net.L)
    G, G0 = taps["G"], taps.get("G0") or {k: np.zeros_like(f64(v)) for k, v in taps["G"].items()}
    Wb = [f64(w) for w in taps["Wb"]]
    links, got = [], {}

    def link(name, tapped, want, tol):
        want = f64(want)
        links.append((name, want, np.broadcast_to(f64(tol) * tol_scale, want.shape)))
        got[name] = f64(tapped)

    # twins, bit for bit
    link("TW Xb", taps["Xb"], round_bf16(taps["X"]), 0.0)
    for l in range(nfw):
        link("TW ab%d" % l, taps["ab"][l], round_bf16(taps["a"][l]), 0.0)
    link("TW dlogb", taps["dlogb"], round_bf16(taps["dlogits"]), 0.0)
    for l in range(L + 1):
        link("TW Wb%d" % l, Wb[l], round_bf16(net.W[l]), 0.0)

    # forward
    xhat, vs, ss = [None] * nfw, [None] * nfw, [None] * nfw
    for l in range(nfw):
        inb = f64(taps["Xb"] if l == 0 else taps["ab"][l - 1])
        want, tol = _contract(inb, Wb[l], net.b[l])
        link("F1 z%d" % l, taps["z"][l], want, tol)
        z = f64(taps["z"][l])
        u = z
        if net.bn:
            (mean, _, rstd), _, _, (tol_mean, tol_rstd) = bn_stat_bounds(taps["z"][l], stat_chunks)
            link("F2 mean%d" % l, taps["mean"][l], mean, tol_mean)
            link("F2 rstd%d" % l, taps["rstd"][l], rstd, tol_rstd)
            xhat[l] = (z - f64(taps["mean"][l])) * f64(taps["rstd"][l])
            u = xhat[l] + net.beta[l]
        v = _nonlin(u, net.nonlin)
        w = v
        if net.l2:
            ss[l] = (v ** 2).mean(axis=1, keepdims=True)
            w = np.where(ss[l] > 1, v / ss[l], v)
        if net.dropout:
            w = w * f64(taps["masks"][l]) / keep
        vs[l] = v
        link("F3 a%d" % l, taps["a"][l], w, ACT_RTOL * np.abs(w) + ACT_ATOL)
    want, tol = _contract(taps["ab"][nact - 1], Wb[L], net.b[L])
    link("F4 logits", taps["logits"], want, tol)

    # loss
    want, tol = criterion(f64(taps["logits"]))
    link("LOSS dlogits", taps["dlogits"], want, tol)

    # backward, from the top
    def sums(key, summands, dead=None, slack=0.0):
        want = G0[key] + f64(summands).sum(axis=0)
        tol = _sum_rule(want) + slack
        if dead is not None:
            tol = np.minimum(1e-4 * max(1.0, float(np.abs(G["W" + key[1:]]).max())),
                             tol + LINK_ULPS * ULP32 * np.abs(f64(summands)).sum(axis=0))
        link("B1 G[%s]" % key, G[key], want, tol)

    want, tol = _contract(f64(taps["ab"][nact - 1]).T, taps["dlogb"], G0["W%d" % L])
    link("B1 G[W%d]" % L, G["W%d" % L], want, tol)
    sums("b%d" % L, taps["dlogits"])
    up, w_up = f64(taps["dlogb"]), Wb[L]
    for l in range(L - 1, nact - 1, -1):  # above the active depth: no gradient
        for k in ("W%d" % l, "b%d" % l) + (("beta%d" % l,) if net.bn else ()):
            link("B1 G[%s] inactive" % k, G[k], G0[k], 0.0)
    for l in range(nact - 1, -1, -1):
        t, e = _contract(up, w_up.T)
        a = f64(taps["a"][l])
        scale = f64(taps["masks"][l]) / keep if net.dropout else 1.0
        dw, e, mag = t * scale, e * scale, np.abs(t) * scale
        if net.l2:
            v, s = vs[l], ss[l]
            lin = lambda d, vv: np.where(s > 1, d / s + vv * (2.0 * (d * vv).sum(axis=1, keepdims=True) / (H * s * s)), d)
            dv = np.where(s > 1, dw / s - v * (2.0 * (dw * v).sum(axis=1, keepdims=True) / (H * s * s)), dw)
            e, mag = lin(e, np.abs(v)), lin(mag, np.abs(v))
            dact = (a > 0).astype(np.float64) if net.nonlin == "relu" else _nonlin_grad(v, net.nonlin)
        else:
            dv = dw
            dact = (a > 0).astype(np.float64) if net.nonlin == "relu" else _nonlin_grad(a * keep, net.nonlin)
        du = dv * dact
        e_du = e * np.abs(dact) + LINK_ULPS * ULP32 * mag
        if net.bn:
            x, r = xhat[l], f64(taps["rstd"][l])
            want = r * (du - du.mean(axis=0) - x * (du * x).mean(axis=0))
            ax, adu = np.abs(x), np.abs(du)
            tol = (r * (e_du + e_du.mean(axis=0) + ax * (e_du * ax).mean(axis=0))
                   + LINK_ULPS * ULP32 * r * (adu + adu.mean(axis=0) + ax * (adu * ax).mean(axis=0)))
            sums("beta%d" % l, du)
        else:
            want, tol = du, e_du
        tol = np.broadcast_to(tol, want.shape) * tol_scale
        lo, hi = round_bf16(want - tol), round_bf16(want + tol)
        links.append(("B2 dzb%d" % l, (lo + hi) / 2, (hi - lo) / 2))
        got["B2 dzb%d" % l] = f64(taps["dzb"][l])
        sums("b%d" % l, want, dead=True if net.bn else None, slack=tol.sum(axis=0) / tol_scale)
        inb = f64(taps["Xb"] if l == 0 else taps["ab"][l - 1])
        want, tol = _contract(inb.T, taps["dzb"][l], G0["W%d" % l])
        link("B1 G[W%d]" % l, G["W%d" % l], want, tol)
        up, w_up = f64(taps["dzb"][l]), Wb[l]
    return links, got


def link_ratios(links, got):
    """{name: worst err / tol} of bf16_links' result; a link of tolerance 0 (bit for bit) counts 0 when equal and inf when not"""
    out = {}
    for name, want, tol in links:
        err = np.abs(got[name] - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / tol)
        out[name] = float(ratio.max()) if ratio.size else 0.0
    return out
