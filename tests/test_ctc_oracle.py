"""The CTC oracle (oracle/ctc_oracle.py) pinned against an independent implementation: torch's CPU ctc_loss with
the blank moved to the last class, as TensorFlow's op has it.  Loss and gradient w.r.t. the logits."""
import numpy as np
import pytest

from oracle.ctc_oracle import ctc_batch, ctc_loss_and_grad, ctc_loss_and_grad_vec


def _torch_ctc(logits, labels):
    import torch
    z = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    lp = torch.log_softmax(z, dim=-1).unsqueeze(1)  # [T, 1, O]
    loss = torch.nn.functional.ctc_loss(lp, torch.tensor([labels], dtype=torch.long), torch.tensor([z.shape[0]]),
                                        torch.tensor([len(labels)]), blank=z.shape[1] - 1, reduction="sum",
                                        zero_infinity=False)
    loss.backward()
    return float(loss.detach()), z.grad.numpy()


CASES = [
    (12, 6, [0, 1, 2]),
    (9, 5, [1, 1, 2, 2]),        # repeated labels need a blank between them
    (7, 4, [0, 0, 0]),           # exactly feasible: T = S + repeats
    (15, 8, []),                 # empty target: all blanks
    (20, 30, [3, 7, 7, 2, 28, 0, 3]),
    (1, 3, [1]),
]


@pytest.mark.parametrize("T,O,labels", CASES)
def test_ctc_oracle_matches_torch(T, O, labels):
    rng = np.random.default_rng(T * 100 + O)
    logits = rng.standard_normal((T, O)) * 2
    loss, grad = ctc_loss_and_grad(logits, labels)
    want_loss, want_grad = _torch_ctc(logits, labels)
    assert np.isfinite(loss)
    np.testing.assert_allclose(loss, want_loss, rtol=1e-10)
    np.testing.assert_allclose(grad, want_grad, rtol=1e-8, atol=1e-12)
    # rows of the gradient sum to zero (softmax minus a distribution over the classes)
    assert np.abs(grad.sum(axis=1)).max() < 1e-10


def test_ctc_oracle_infeasible_and_batch():
    rng = np.random.default_rng(3)
    loss, grad = ctc_loss_and_grad(rng.standard_normal((3, 5)), [1, 1, 2])  # needs 4 frames
    assert loss == np.inf and not grad.any()
    logits = rng.standard_normal((11 + 6, 7))
    total, grad, n_labels = ctc_batch(logits, [11, 6], [0, 1, 2, 5, 5], [3, 2])
    l0, g0 = ctc_loss_and_grad(logits[:11], [0, 1, 2])
    l1, g1 = ctc_loss_and_grad(logits[11:], [5, 5])
    assert n_labels == 5 and np.isclose(total, l0 + l1)
    assert (grad[:11] == g0).all() and (grad[11:] == g1).all()


# ---- the vectorised oracle (ctc_loss_and_grad_vec): the same recursion, one numpy step per frame ----

@pytest.mark.parametrize("T,O,labels", CASES + [
    (30, 4, [0, 0, 1, 1, 1, 2, 0, 0, 2, 2]),   # repeats everywhere
    (1, 5, []),                                # S = 0 on one frame
    (6, 9, [0, 1, 2, 3, 4, 5]),                # T = S: every frame emits a label
    (8, 4, [0, 0, 1, 1, 2]),                   # T = S + repeats, again exactly feasible
    (5, 9, [0, 1, 2, 3, 4, 5]),                # one frame short
    (7, 4, [0, 0, 1, 1, 2]),                   # one frame short with repeats
    (0, 6, []),                                # no frames, no labels
    (0, 6, [2, 3]),                            # no frames, labels
])
@pytest.mark.parametrize("scale", [2.0, 25.0])
def test_vectorised_oracle_equals_the_scalar_one(T, O, labels, scale):
    rng = np.random.default_rng(T * 100 + O)
    logits = rng.standard_normal((T, O)) * scale
    loss, grad = ctc_loss_and_grad(logits, labels)
    vloss, vgrad = ctc_loss_and_grad_vec(logits, labels)
    assert vgrad.shape == grad.shape == (T, O) and vgrad.dtype == np.float64
    feasible = T >= len(labels) + sum(a == b for a, b in zip(labels, labels[1:])) if T else not labels
    assert np.isfinite(loss) == feasible
    if feasible:
        np.testing.assert_allclose(vloss, loss, rtol=1e-12, atol=0)
    else:
        assert vloss == loss == np.inf and not grad.any()
    np.testing.assert_allclose(vgrad, grad, rtol=0, atol=1e-12)


def test_oracles_without_frames():
    """T = 0: only the empty labelling is possible (ctc.h says the same of the device)"""
    for fn in (ctc_loss_and_grad, ctc_loss_and_grad_vec):
        loss, grad = fn(np.zeros((0, 5)), [])
        assert loss == 0.0 and grad.shape == (0, 5)
        loss, grad = fn(np.zeros((0, 5)), [1, 2])
        assert loss == np.inf and grad.shape == (0, 5)
    logits = np.random.default_rng(8).standard_normal((9, 5))
    for fast in (False, True):
        total, grad, n_labels = ctc_batch(logits, [0, 9, 0, 0], [1, 2, 1], [0, 3, 0, 0], fast=fast)
        want, g = ctc_loss_and_grad(logits, [1, 2, 1])
        assert total == want and n_labels == 3 and (grad == g).all()
        assert ctc_batch(logits, [0, 9, 0, 0], [1, 2, 1, 3], [0, 3, 1, 0], fast=fast)[0] == np.inf


def test_ctc_batch_fast_switch():
    rng = np.random.default_rng(5)
    logits = rng.standard_normal((11 + 3 + 6, 7)) * 4
    args = (logits, [11, 3, 6], [0, 1, 2, 1, 1, 2, 5, 5], [3, 3, 2])  # (the middle utterance is one frame short)
    total, grad, n = ctc_batch(*args)
    ftotal, fgrad, fn = ctc_batch(*args, fast=True)
    assert total == ftotal == np.inf and n == fn == 8
    assert not fgrad[11:14].any() and fgrad[:11].any() and fgrad[14:].any()
    np.testing.assert_allclose(fgrad, grad, rtol=0, atol=1e-12)


@pytest.mark.parametrize("S,scale,atol", [(255, 2.0, 1e-12), (511, 2.0, 1e-12), (511, 12.0, 1e-10)])
def test_vectorised_oracle_matches_torch_at_the_largest_sizes(S, scale, atol):
    """255 and 511 labels (511 and 1023 states: the two largest register tiles of the device kernel), a quarter of the
    positions repeating their neighbour; neither oracle had been compared with anything at this size.
    The peaky case (scale 12, the regime of a trained model): alpha + beta - log Z is a difference of numbers of
    magnitude ~1.5e4 there, which float64 resolves to 2^-52 * 1.5e4 = 3e-12 -- a posterior near 1 carries a few of those
    roundings in either implementation, hence atol 1e-10 for it instead of the file's 1e-12."""
    rng = np.random.default_rng(S)
    O = 36
    labels = rng.integers(0, O - 1, size=S)
    rep = rng.random(S) < 0.25
    rep[0] = False
    for i in np.flatnonzero(rep):
        labels[i] = labels[i - 1]
    T = 2 * S + 40
    logits = rng.standard_normal((T, O)) * scale
    loss, grad = ctc_loss_and_grad_vec(logits, labels)
    want_loss, want_grad = _torch_ctc(logits, [int(x) for x in labels])
    assert np.isfinite(loss)
    np.testing.assert_allclose(loss, want_loss, rtol=1e-10)
    np.testing.assert_allclose(grad, want_grad, rtol=1e-8, atol=atol)
    assert np.abs(grad.sum(axis=1)).max() < 1e-10
