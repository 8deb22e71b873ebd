"""Batch norm's backward inside the dA blocks of the fp32-emulating dual launch (csrc/gemm_bf16.hip: EPI_DACT_BN, epilogue_dact_bn;
csrc/hb_math.h: the arithmetic it shares with hb_apply_kernel; switch TFK_X3_FUSE_BNB, read when an engine is created).

The fused epilogue must change NOTHING: for every shape, three consecutive optimiser steps (so that the launches' generation
tags and the alternating sets of sync words are exercised) of a fresh engine with the switch at 1 (fused where the launch
finds it safe) and of one with the switch at 2 (the launch always decides UNFUSED: the fallback a single process never takes
otherwise) are compared with an engine with the switch at 0 (the separate apply kernel, as before), after every step:
  * tfk_param_checksum of the parameter arena, of the bias / beta vectors and of the three-plane twins: equal;
  * the loss: bit for bit;
  * the bias, beta and weight gradients of the hidden layers: bit for bit.

Shapes.  F = 40, O = 48, L = 2; H = 256 and H = 160 (a ragged block column); T = 128 (one row tile: a rendezvous of one), 256
(two), 200 (ragged last tile; the apply kernel cuts 200 rows into 7 chunks of 29, which do not tile 128 rows: the rule declines it
and the test says so) and 1024 once.  The dual launch itself needs 256 tiles between dA and dW (gemm_bf16x3_dual), which those
widths never have -- so the same frame counts are run at H = 2048 and H = 2000 (ragged block column, 16 x 16 tiles of dW) as
well, where the launch under test really runs; L = 3 there once, for two such launches per step."""
import os

import numpy as np
import pytest

from util import batch, engine_grads, make_pair

pytestmark = pytest.mark.gpu

F, O = 40, 48


def _chunk_rows(T, rows=32):
    rs = min(max(-(-T // rows), 1), 256)
    return -(-T // rs)


def _eligible(T, H):
    """csrc/x3_layout.h: dual_bnb_eligible for the hidden-to-hidden launch of an unstacked pass (K of dA = H)"""
    return 128 % _chunk_rows(T) == 0 and T <= H and -(-T // 128) <= 32


def _engine(switch, T, H, L, nonlin):
    old = os.environ.get("TFK_X3_FUSE_BNB")
    os.environ["TFK_X3_FUSE_BNB"] = str(switch)
    try:
        eng, _ = make_pair(np.random.default_rng(7), input_dim=F, num_layers=L, num_units=H, output_dim=O, nonlin=nonlin,
                           batch_norm=True, init_learning_rate=1e-3, num_steps=10, max_frames=T, compute_dtype="float32")
    finally:
        if old is None:
            del os.environ["TFK_X3_FUSE_BNB"]
        else:
            os.environ["TFK_X3_FUSE_BNB"] = old
    return eng


def _run(switch, T, H, L, nonlin, profile=False):
    """three optimiser steps: per step (loss bits, checksums, hidden-layer gradients), and the profile of the last step"""
    eng = _engine(switch, T, H, L, nonlin)
    rng = np.random.default_rng(11)
    out, prof = [], None
    try:
        for step in range(3):
            X, y = batch(rng, T, F, O)
            if profile and step == 2:
                eng.profile_begin()
            eng.accumulate(X, y)
            if profile and step == 2:
                prof = eng.profile_end()
            g = engine_grads(eng)
            grads = {k: v.copy() for k, v in g.items() if k[-1] != str(L) or k.startswith("beta")}
            loss = np.float32(eng.apply())
            out.append((loss.view(np.uint32), [eng.param_checksum(w) for w in (0, 2, 3)], grads))
    finally:
        eng.close()
    return out, prof


def _compare(label, ref, got):
    for step, ((l0, c0, g0), (l1, c1, g1)) in enumerate(zip(ref, got)):
        assert c0 == c1, "%s step %d: parameter checksums differ" % (label, step)
        assert l0 == l1, "%s step %d: loss bits %08x against %08x" % (label, step, l1, l0)
        assert set(g0) == set(g1)
        for k in sorted(g0):
            assert np.array_equal(g0[k].view(np.uint32), g1[k].view(np.uint32)), "%s step %d: gradient %s differs in %d places" % (
                label, step, k, int((g0[k].view(np.uint32) != g1[k].view(np.uint32)).sum()))


CASES = [(T, H, 2, nonlin) for H in (256, 160) for T in (128, 256, 200) for nonlin in ("relu", "tanh")]
CASES += [(1024, 256, 2, "relu")]
# where the dual launch runs (at least 256 tiles of 128 x 128 between dA and dW)
CASES += [(128, 2048, 2, "relu"), (256, 2048, 2, "tanh"), (200, 2048, 2, "relu"), (256, 2000, 2, "relu"), (1000, 2000, 2, "tanh"),
          (1024, 2048, 3, "relu")]


@pytest.mark.parametrize("T,H,L,nonlin", CASES)
def test_fused_and_forced_fallback_equal_the_separate_apply_kernel(T, H, L, nonlin):
    if T == 200:
        assert not _eligible(T, H), "200 frames: 7 chunks of 29 rows do not tile the 128-row tile; the rule must decline"
    elif H >= 2000:
        assert _eligible(T, H)
    ref, _ = _run(0, T, H, L, nonlin)
    assert all(np.isfinite(l.view(np.float32)) for l, _, _ in ref)
    for switch, what in ((1, "fused"), (2, "forced UNFUSED")):
        got, _ = _run(switch, T, H, L, nonlin)
        _compare("T %d H %d L %d %s, %s" % (T, H, L, nonlin, what), ref, got)


@pytest.mark.parametrize("T,H,L", [(256, 2048, 3), (1000, 2000, 2)])
def test_fused_run_still_launches_hidden_backward_once_per_layer(T, H, L):
    """The apply kernel stays enqueued behind every dual launch (its blocks return when the launch did the work): the engine's
    profile counts it once per hidden layer, fused or not, and the dual launch once per layer boundary it covers.

    And the fused path really RUNS here -- the bitwise comparison above would also pass if the host or the kernel quietly fell
    back.  While profiling, the engine copies the mode word every EPI_DACT_BN launch leaves (FUSED or UNFUSED, decided on the
    device) and books the apply kernel's bytes accordingly: nothing for an apply launch whose pass the dA blocks did, and
    6 B per element more for that dual launch (z read, three planes of dz written, du not written).  With O = 48 the output
    layer's pair has too few tiles for a dual launch, so the top hidden layer's apply kernel always works; the L - 1 below it
    sit behind eligible dual launches: fused with the switch at 1, never with it at 2 (forced UNFUSED) or 0."""
    prof = {sw: _run(sw, T, H, L, "relu", profile=True)[1] for sw in (1, 2, 0)}
    count = lambda p, name: sum(s["launches"] for s in p if name in s["name"])  # noqa: E731
    moved = lambda p, name: sum(s["bytes"] for s in p if name in s["name"])  # noqa: E731
    names = sorted(s["name"] for s in prof[1])
    for sw in (1, 2, 0):
        assert count(prof[sw], "hidden_backward") == L, (sw, names)
        assert count(prof[sw], "dual(dA+dW)") == L - 1, (sw, names)
    full = 28.0 * T * H
    assert moved(prof[0], "hidden_backward") == L * full
    assert moved(prof[2], "hidden_backward") == L * full, "forced UNFUSED: every apply kernel does its pass"
    assert moved(prof[1], "hidden_backward") == full, "the %d apply launches behind EPI_DACT_BN launches found their pass done" % (L - 1)
    assert moved(prof[1], "dual(dA+dW)") == moved(prof[0], "dual(dA+dW)") + (L - 1) * 6.0 * T * H
    assert moved(prof[2], "dual(dA+dW)") == moved(prof[0], "dual(dA+dW)")
    for sw, what in ((1, "fused"), (2, "forced UNFUSED"), (0, "switch 0")):
        for s in prof[sw]:
            if s["name"] == "hidden_backward" or "dual" in s["name"]:
                print("x3-dual-bnb profile T %d H %d: %-22s %d launches, %.1f us each, %.1f MB (%s)" % (
                    T, H, s["name"], s["launches"], 1e3 * s["total_ms"] / s["launches"], s["bytes"] / 1e6, what))
