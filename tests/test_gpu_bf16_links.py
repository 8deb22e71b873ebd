"""Mixed-precision mode (TFK_DTYPE_BF16) link by link on the engine's OWN operands: the sharp check of that mode.

The whole-network bf16 tests (tests/test_gpu_bf16_mode.py and the bf16 legs of the CTC files) allow 2e-3 by norm because an
operand within fp32 round-off of a bf16 rounding boundary rounds the other way in the engine than in the oracle and batch norm
spreads it (tests/test_bf16_links_host.py shows that cascade on the CPU).  Here every link of the chain -- each contraction, the
statistics, the activation chain, the loss gradient, BN backward, every gradient sum -- is restated in float64 on the bf16 twins
and fp32 tensors the engine itself stored (tfk_debug_fetch_twin, tfk_debug_capture), so both sides read bit-identical values, no
flip is possible and every bound is an fp32 round-off bound (oracle/dnn_oracle.py: bf16_links states and derives them); the
twins themselves are compared bit for bit with the RNE rounding of the fp32 tensor beside them.  The cases reach every tile and
twin edge of the bf16 path at the smallest size that does; a micro-batch has at most 257 frames.  One line per link kind and
case under `pytest -s` (recorded in profiles/bf16_links_edges.txt).  A ratio above 1 is a finding, not a tolerance to widen."""
import numpy as np
import pytest

from oracle.dnn_oracle import ctc_criterion, round_bf16, xent_criterion
from test_ctc_mmi_host import mmi_loss_grad64, mmi_tol
from util import assert_links, batch, engine_grads, engine_link_taps, engine_params, make_pair

pytestmark = pytest.mark.gpu

NET = dict(input_dim=20, num_units=64, output_dim=9, init_learning_rate=1e-3, num_steps=50)
UTT = [60, 35, 48]
T0 = sum(UTT)
CHAINS = {
    "tanh-bn": dict(nonlin="tanh", batch_norm=True),
    "relu-bn": dict(nonlin="relu", batch_norm=True),
    "sigmoid-l2": dict(nonlin="sigmoid", l2_norm=True),
    "relu-bn-drop": dict(nonlin="relu", batch_norm=True, keep_prob=0.7),
    "relu": dict(nonlin="relu"),
}


def _pair(seed, max_frames=320, **kw):
    rng = np.random.default_rng(seed)
    eng, net = make_pair(rng, max_frames=max_frames, compute_dtype="bfloat16", **kw)
    eng.debug_capture(True)
    return rng, eng, net


def _lexicon():
    """the lexicon and references of tests/test_gpu_ctc_mmi.py's engine case"""
    from tfkaldi_amd.neuralNetworks.ctc_lm import GraphLM
    words = [np.array(w, np.int32) for w in ([0, 1, 2], [0, 3], [4, 4, 5], [6], [2, 1])]
    lex = GraphLM.from_lexicon(words, 8, 7, word_logprob=[-1.0, -0.5, -2.0, -1.5, -0.7])
    sep = np.array([7], np.int32)
    refs = [np.concatenate([words[0], sep, words[2]]), words[3], np.concatenate([words[4], sep, words[1], sep, words[3]])]
    return lex, refs


def mmi_criterion(utt, refs, lex, lam, cw):
    """dLogits of the MMI criterion restated on the logits handed in, utterance by utterance, under mmi_tol's gradient bound"""
    def crit(z):
        want, tol = [], []
        for zu, ref in zip(np.split(z, np.cumsum(utt)[:-1]), refs):
            want.append(mmi_loss_grad64(zu, ref, lex, lam, cw)[1])
            tol.append(np.full(zu.shape, mmi_tol(zu, lex, lam, cw)["grad"]))
        return np.concatenate(want), np.concatenate(tol)
    return crit


def _run(eng, X, crit_name, y=None):
    """one training micro-batch under the criterion; returns the link checker's criterion"""
    lex, refs = _lexicon()
    labels, lab = np.concatenate(refs).astype(np.int32), np.array([r.size for r in refs], np.int32)
    if crit_name == "xent":
        eng.accumulate(X, y)
        return xent_criterion(y)
    if crit_name == "ctc":
        eng.accumulate_ctc(X, UTT, labels, lab)
        return ctc_criterion(UTT, labels, lab)
    eng.ctc_set_den(lex)
    eng.accumulate_ctc_mmi(X, UTT, labels, lab, lm_scale=0.6, ctc_weight=0.3)
    return mmi_criterion(UTT, refs, lex, 0.6, 0.3)


@pytest.mark.parametrize("crit", ["xent", "ctc", "mmi"])
@pytest.mark.parametrize("chain,L", [("tanh-bn", 4), ("relu-bn", 6)])
def test_depth_under_every_criterion(gpu, chain, L, crit):
    """four layers of tanh + batch norm -- the depth tests/test_gpu_ctc_mmi.py had to drop from its whole-network bf16 case --
    and the six layers of cfg3, under the cross-entropy, the CTC loss and MMI (the CTC gradient kernels write the dLogits twin)"""
    rng, eng, net = _pair(7100 + L, num_layers=L, **dict(NET, **CHAINS[chain]))
    X, y = batch(rng, T0, NET["input_dim"], NET["output_dim"])
    criterion = _run(eng, X, crit, y)
    assert_links("%s L%d %s" % (chain, L, crit), net, engine_link_taps(eng, net, X), criterion)
    eng.close()


@pytest.mark.parametrize("chain,L,dims", [
    ("relu-bn", 3, dict(input_dim=22, num_units=37, output_dim=13)),  # no dimension % 8 == 0: padding columns in every twin
    ("relu-bn", 3, dict(input_dim=22, num_units=36, output_dim=13)),  # a leading dimension of 36: the packed shadow
    ("sigmoid-l2", 4, {}),                                            # act_backward_rows
    ("relu-bn-drop", 4, {}),                                          # masks; the fused backward reads them off the output
    ("relu", 4, {}),                                                  # no batch norm: the non-fused backward
], ids=["odd-dims", "packed-shadow", "sigmoid-l2", "relu-bn-drop", "relu-plain"])
def test_chains(gpu, chain, L, dims):
    kw = dict(NET, num_layers=L, **dict(CHAINS[chain], **dims))
    rng, eng, net = _pair(7200 + L + len(chain), **kw)
    X, y = batch(rng, T0, kw["input_dim"], kw["output_dim"])
    eng.accumulate(X, y)
    taps = engine_link_taps(eng, net, X)
    assert_links("%s L%d F%d H%d" % (chain, L, kw["input_dim"], kw["num_units"]), net, taps, xent_criterion(y))
    if net.dropout:
        assert all(0.5 < m.mean() < 0.9 for m in taps["masks"])
    eng.close()


@pytest.mark.parametrize("cfg", [3, 4, 5, 6])
@pytest.mark.parametrize("T,H", [(129, 64), (129, 130), (257, 64), (257, 130)])
def test_forced_tiles_inside_a_full_step(gpu, T, H, cfg):
    """the 128 x 128 and 256 x 128 tiles that only cfg3 / cfg4 sizes select, forced onto a small step: one row and two columns
    past a tile, through the statistics epilogue, the activation-derivative epilogue and the dual launch"""
    from tfkaldi_amd import _lib
    lib = _lib.load()
    kw = dict(NET, num_layers=2, num_units=H, **CHAINS["relu-bn"])
    rng, eng, net = _pair(7300 + T + H, **kw)
    X, y = batch(rng, T, kw["input_dim"], kw["output_dim"])
    try:
        lib.tfk_gemm_bf16_force_config(cfg)
        eng.accumulate(X, y)
        eng.synchronize()
    finally:
        lib.tfk_gemm_bf16_force_config(-1)
    assert_links("relu-bn L2 T%d H%d cfg%d" % (T, H, cfg), net, engine_link_taps(eng, net, X), xent_criterion(y),
                 stat_chunks=(64, 128, 256) if cfg == 5 else (64, 128))
    eng.close()


def _sync(net, eng):
    """the oracle object takes the engine's parameters (the link checker reads W, b, beta from it)"""
    p = engine_params(eng)
    for l in range(net.L + 1):
        net.W[l], net.b[l] = p["W%d" % l].astype(np.float64), p["b%d" % l].astype(np.float64)
    if net.bn:
        for l in range(net.L):
            net.beta[l] = p["beta%d" % l].astype(np.float64)


def test_layerwise_growth(gpu):
    """step, add_layer, init_last_layer, step, step: the shadow after the control ops, and hidden layers above the active depth
    evaluated in training mode (their outputs and twins are links too; their gradient sums must stay zero)"""
    kw = dict(NET, num_layers=3, layerwise_init=True, **CHAINS["tanh-bn"])
    rng, eng, net = _pair(7400, **kw)
    X, y = batch(rng, T0, kw["input_dim"], kw["output_dim"])
    eng.accumulate(X, y)
    assert net.num_active() == 1
    assert_links("layerwise depth 1", net, engine_link_taps(eng, net, X), xent_criterion(y))
    eng.apply()
    eng.add_layer()
    net.add_layer()
    eng.init_last_layer()
    _sync(net, eng)
    assert not net.W[net.L].any() and net.num_active() == 2
    eng.accumulate(X, y)
    assert_links("layerwise depth 2 after init", net, engine_link_taps(eng, net, X), xent_criterion(y))
    # the output layer is zero there, so every hidden dz is zero and the backward links hold trivially: one optimiser step
    # later it is not, and hidden_backward and the dual launch run at depth 2 with an inactive layer above them
    eng.apply()
    _sync(net, eng)
    assert net.W[net.L].any()
    eng.accumulate(X, y)
    taps = engine_link_taps(eng, net, X)
    assert all(d.any() for d in taps["dzb"]) and len(taps["dzb"]) == 2 and len(taps["z"]) == 3
    assert_links("layerwise depth 2, second step", net, taps, xent_criterion(y))
    eng.close()


@pytest.mark.parametrize("dims,mirrored", [(dict(output_dim=16), True), (dict(input_dim=22, num_units=36, output_dim=13), False)],
                         ids=["mirrored-shadow", "packed-shadow"])
def test_two_microbatches_then_the_optimiser(gpu, dims, mirrored):
    """G after the second micro-batch = G after the first + the links' g; then tfk_apply: where the shadow mirrors the arena
    (every leading dimension a multiple of 8: 64 units, 16 outputs) adam_kernel writes it with the update and it must be the RNE
    rounding of the new parameters bit for bit; a packed shadow (a leading dimension of 36) is refused as stale until the next pass has rebuilt it"""
    from tfkaldi_amd import _lib
    from tfkaldi_amd._lib import EngineError
    kw = dict(NET, num_layers=3, **dict(CHAINS["tanh-bn"], **dims))
    rng, eng, net = _pair(7500, **kw)
    X, y = batch(rng, T0, kw["input_dim"], kw["output_dim"])
    X2, y2 = batch(rng, 97, kw["input_dim"], kw["output_dim"])
    eng.accumulate(X, y)
    assert_links("first micro-batch", net, engine_link_taps(eng, net, X), xent_criterion(y))
    G1 = engine_grads(eng)
    eng.accumulate(X2, y2)
    assert_links("second micro-batch", net, engine_link_taps(eng, net, X2, G0=G1), xent_criterion(y2))
    eng.apply()
    _sync(net, eng)
    if not mirrored:
        with pytest.raises(EngineError, match="shadow is not current"):
            eng.debug_fetch_twin(_lib.TWIN_WEIGHTS, 0)
    else:
        for l in range(net.L + 1):
            got = eng.debug_fetch_twin(_lib.TWIN_WEIGHTS, l)
            assert np.array_equal(got, round_bf16(net.W[l])), "shadow of layer %d as adam_kernel wrote it" % l
    eng.accumulate(X, y)
    assert_links("after the optimiser step", net, engine_link_taps(eng, net, X), xent_criterion(y))
    eng.close()


def test_taps_refuse_by_name(gpu):
    from tfkaldi_amd import _lib
    from tfkaldi_amd._lib import EngineError
    rng = np.random.default_rng(7600)
    kw = dict(NET, num_layers=2, **CHAINS["relu-bn"])
    X, y = batch(rng, 40, kw["input_dim"], kw["output_dim"])
    eng, _ = make_pair(rng, max_frames=64, compute_dtype="bfloat16", **kw)
    eng.accumulate(X, y)
    with pytest.raises(EngineError, match="capture is off"):
        eng.debug_fetch(_lib.DBG_DPREACT, 0, 40)
    with pytest.raises(EngineError, match="capture is off"):
        eng.debug_fetch_twin(_lib.TWIN_DPREACT, 0, 40)
    eng.debug_capture(True)
    with pytest.raises(EngineError, match="no captured dz"):
        eng.debug_fetch(_lib.DBG_DPREACT, 0, 40)
    eng.accumulate(X, y)
    assert eng.debug_fetch(_lib.DBG_DPREACT, 0, 40).any()
    eng.eval_accumulate(X, y)
    with pytest.raises(EngineError, match="training calls only"):
        eng.debug_fetch_twin(_lib.TWIN_DLOGITS, 0, 40)
    with pytest.raises(EngineError, match="no captured dz"):
        eng.debug_fetch_twin(_lib.TWIN_DPREACT, 0, 40)
    eng.debug_capture(False)
    eng.close()
    for dtype, what in (("float32", "three-plane"), ("float32_mfma", "bf16 mode only")):
        eng, _ = make_pair(rng, max_frames=64, compute_dtype=dtype, **kw)
        with pytest.raises(EngineError, match=what):
            eng.debug_fetch_twin(_lib.TWIN_WEIGHTS, 0)
        with pytest.raises(EngineError, match="emulated-fp32" if dtype == "float32" else "bf16 mode only"):
            eng.debug_capture(True)
        eng.close()


def test_capture_off_enqueues_the_parents_launches(gpu):
    """the engine's profile of a training step: the same kernel families and launch counts with capture never switched on, switched
    on and off again; switched on, the only difference is none the profile sees (the copies are not kernels)"""
    rng = np.random.default_rng(7700)
    kw = dict(NET, num_layers=3, **CHAINS["tanh-bn"])
    X, y = batch(rng, T0, kw["input_dim"], kw["output_dim"])
    eng, _ = make_pair(rng, max_frames=320, compute_dtype="bfloat16", **kw)

    def profile():
        eng.profile_begin()
        eng.accumulate(X, y, last=True)
        eng.apply()
        return sorted((s["name"], s["launches"]) for s in eng.profile_end())
    eng.accumulate(X, y)
    eng.apply()
    never = profile()
    eng.debug_capture(True)
    on = profile()
    eng.debug_capture(False)
    off = profile()
    assert never == off == on and never
    eng.close()
