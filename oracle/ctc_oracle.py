"""CPU oracle of the CTC loss (test infrastructure: imported by tests/ only, never by the product).

What it restates: the loss the reference's CTCTrainer means to build -- `tf.nn.ctc_loss(tf.pack(logits),
sparse_targets, logit_seq_length)` (neuralNetworks/trainer.py:558-570) -- with TensorFlow's conventions for that op:
time-major logits, the BLANK is the LAST class (num_classes - 1), repeated labels are merged
(ctc_merge_repeated=True), labels are not pre-collapsed, and the per-sequence loss is -log p(labels | logits).
The reference's own method cannot run (it iterates `range(len(batch_size))` over an int, fills the sparse values from
the logits and returns nothing), so there is no reference behaviour to pin: **parity unpinned**.  The
arithmetic below is the published algorithm (Graves et al. 2006, "Connectionist Temporal Classification", eqs. 6-16,
in log space) and is pinned against an independent implementation, torch.nn.functional.ctc_loss on CPU
(tests/test_ctc_oracle.py).

Trainer conventions that DO come from the reference (neuralNetworks/trainer.py:126-133, 165-169, 174-175, 198):
batch_loss is the SUM of the per-utterance losses and num_frames counts TARGET labels, so the reported average loss
and the mean gradient divide by the number of labels of the step.
"""
import numpy as np


def _logsumexp(*xs):
    m = np.max(xs)
    if not np.isfinite(m):
        return m
    return m + np.log(sum(np.exp(x - m) for x in xs))


def log_softmax(z):
    z = z - z.max(axis=-1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=-1, keepdims=True))


def ctc_loss_and_grad(logits, labels, blank=None):
    """logits [T, O] float64, labels [S] ints in [0, O-1) -> (loss, d loss / d logits [T, O]).
    An utterance too short for its labels has loss +inf and a zero gradient.  Without frames (T = 0) only the empty
    labelling is possible: loss 0 for S = 0, +inf otherwise, and the gradient is empty (what ctc.h states for the device)."""
    logits = np.asarray(logits, dtype=np.float64)
    T, O = logits.shape
    blank = O - 1 if blank is None else blank
    labels = [int(x) for x in labels]
    assert all(0 <= x < O and x != blank for x in labels)
    if T == 0:
        return (0.0 if not labels else np.inf), np.zeros_like(logits)
    ext = [blank]
    for x in labels:
        ext += [x, blank]
    n = len(ext)
    logp = log_softmax(logits)
    ninf = -np.inf

    def skip_ok(s):  # transition s-2 -> s allowed
        return s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]

    alpha = np.full((T, n), ninf)
    alpha[0, 0] = logp[0, ext[0]]
    if n > 1:
        alpha[0, 1] = logp[0, ext[1]]
    for t in range(1, T):
        for s in range(n):
            terms = [alpha[t - 1, s]]
            if s >= 1:
                terms.append(alpha[t - 1, s - 1])
            if skip_ok(s):
                terms.append(alpha[t - 1, s - 2])
            alpha[t, s] = _logsumexp(*terms) + logp[t, ext[s]]
    log_z = _logsumexp(alpha[T - 1, n - 1], alpha[T - 1, n - 2]) if n > 1 else alpha[T - 1, 0]
    if not np.isfinite(log_z):
        return np.inf, np.zeros_like(logits)
    beta = np.full((T, n), ninf)
    beta[T - 1, n - 1] = logp[T - 1, ext[n - 1]]
    if n > 1:
        beta[T - 1, n - 2] = logp[T - 1, ext[n - 2]]
    for t in range(T - 2, -1, -1):
        for s in range(n):
            terms = [beta[t + 1, s]]
            if s + 1 < n:
                terms.append(beta[t + 1, s + 1])
            if s + 2 < n and skip_ok(s + 2):
                terms.append(beta[t + 1, s + 2])
            beta[t, s] = _logsumexp(*terms) + logp[t, ext[s]]
    grad = np.exp(logp)  # softmax
    for t in range(T):
        for s in range(n):
            v = alpha[t, s] + beta[t, s]
            if np.isfinite(v):
                grad[t, ext[s]] -= np.exp(v - logp[t, ext[s]] - log_z)
    return -log_z, grad


def _lse3(a, b, c):
    """elementwise log(e^a + e^b + e^c) with true -inf (all three -inf -> -inf)"""
    m = np.maximum(a, np.maximum(b, c))
    ok = np.isfinite(m)
    ms = np.where(ok, m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(ok, ms + np.log(np.exp(a - ms) + np.exp(b - ms) + np.exp(c - ms)), -np.inf)


def ctc_loss_and_grad_vec(logits, labels, blank=None):
    """ctc_loss_and_grad with the recursion vectorised over the states: one Python loop over t per sweep instead of one
    over (t, s).  Same arithmetic (float64, true -inf), same return contract; fast enough for 511 labels (1023 states)."""
    logits = np.asarray(logits, dtype=np.float64)
    T, O = logits.shape
    blank = O - 1 if blank is None else blank
    labels = np.asarray([int(x) for x in labels], dtype=np.int64)
    assert ((0 <= labels) & (labels < O) & (labels != blank)).all()
    if T == 0:
        return (0.0 if labels.size == 0 else np.inf), np.zeros_like(logits)
    n = 2 * labels.size + 1
    ext = np.full(n, blank, dtype=np.int64)
    ext[1::2] = labels
    skip = np.zeros(n, dtype=bool)  # transition s-2 -> s allowed
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    logp = log_softmax(logits)
    lpe = logp[:, ext]  # [T, n]: log p_t(state)
    ninf = -np.inf

    alpha = np.full((T, n), ninf)
    alpha[0, :2] = lpe[0, :2]
    p1, p2 = np.full(n, ninf), np.full(n, ninf)
    for t in range(1, T):
        a = alpha[t - 1]
        p1[1:] = a[:-1]
        p2[2:] = np.where(skip[2:], a[:-2], ninf)
        alpha[t] = _lse3(a, p1, p2) + lpe[t]
    log_z = float(_lse3(alpha[T - 1, n - 1], alpha[T - 1, n - 2] if n > 1 else ninf, ninf))
    if not np.isfinite(log_z):
        return np.inf, np.zeros_like(logits)
    beta = np.full((T, n), ninf)
    beta[T - 1, max(n - 2, 0):] = lpe[T - 1, max(n - 2, 0):]
    q1, q2 = np.full(n, ninf), np.full(n, ninf)
    for t in range(T - 2, -1, -1):
        b = beta[t + 1]
        q1[:-1] = b[1:]
        q2[:-2] = np.where(skip[2:], b[2:], ninf)
        beta[t] = _lse3(b, q1, q2) + lpe[t]
    v = alpha + beta
    ok = np.isfinite(v)
    gamma = np.where(ok, np.exp(np.where(ok, v - lpe - log_z, 0.0)), 0.0)  # state posteriors [T, n]
    grad = np.exp(logp)  # softmax
    np.subtract.at(grad, (np.arange(T)[:, None], ext[None, :]), gamma)  # states of one class in ascending order
    return -log_z, grad


def ctc_batch(logits, utt_len, labels, label_len, fast=False):
    """flat utterance-major logits [sum(utt_len), O], concatenated labels -> (sum of losses, gradient, #labels);
    fast: the vectorised recursion (ctc_loss_and_grad_vec) instead of the scalar one"""
    logits = np.asarray(logits, dtype=np.float64)
    grad = np.zeros_like(logits)
    total, r, q = 0.0, 0, 0
    one = ctc_loss_and_grad_vec if fast else ctc_loss_and_grad
    for n_t, n_s in zip(utt_len, label_len):
        loss, g = one(logits[r:r + n_t], labels[q:q + n_s])
        total += loss
        grad[r:r + n_t] = g
        r += n_t
        q += n_s
    return total, grad, int(np.sum(label_len))
