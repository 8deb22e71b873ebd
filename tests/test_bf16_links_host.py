"""The link checker of the mixed-precision step (oracle/dnn_oracle.py: bf16_links) without a GPU.  A float32 numpy restatement
of the step -- the engine's algebra with every intermediate in np.float32, bf16 twins where the engine has them -- stands in for
the engine and produces the taps.  Its reductions are ACCUMULATED in float32 in the orders the engine's kernels use (Fp32Sums:
k-steps of 16 and 64-k tiles in a contraction, reduction trees for column sums, tiled two-pass statistics merged after Chan);
a second form rounds every reduction once from its exact value (ExactSums), the least round-off the format allows, as a lower
envelope.  Three things are shown:

  * the cascade is real and the links are immune to it: on a fixed net the restatement's whole-network gradients are more than
    1e-4 (relative Frobenius) from OracleDNN(gemm_dtype="bfloat16"), although both are correct -- an operand within fp32
    round-off of a bf16 rounding boundary rounds the other way, batch norm spreads it -- and every link still holds; even the
    exactly rounded form cascades;
  * the tolerances come from the arithmetic and leave head-room: over 20 seeds x 5 chains x 3 depths the fp32-accumulating
    restatement uses at most a quarter (HEADROOM) of every bound but two, which are named, explained and asserted at the bound
    itself (test_every_link_leaves_headroom), and the exactly rounded form a quarter of every bound;
  * seven subtly wrong steps each fail a link, and the test names which one: the evidence that tests/test_gpu_bf16_links.py would
    notice such a kernel -- with the limit of the dz twin's interval check measured on random elements."""
import numpy as np
import pytest

from oracle.dnn_oracle import OracleDNN, bf16_links, ctc_criterion, link_ratios, round_bf16, xent_criterion
from util import randomize

F_IN, H, O, T = 20, 64, 9, 143
UTT, LABELS, LABEL_LEN = [60, 35, 48], np.array([0, 1, 2, 7, 4, 4, 5, 6, 2, 1, 7, 0, 3, 7, 6], np.int32), [7, 1, 7]
CHAINS = {
    "tanh": dict(nonlin="tanh", batch_norm=True),
    "relu": dict(nonlin="relu", batch_norm=True),
    "sigmoid-l2": dict(nonlin="sigmoid", l2_norm=True),
    "relu-drop": dict(nonlin="relu", batch_norm=True, keep_prob=0.7),
    "relu-plain": dict(nonlin="relu"),
}
HEADROOM = 0.25
f32 = np.float32


def _twin(x):
    """the bf16 twin of an fp32 array, as an fp32 array of the same values"""
    return round_bf16(x).astype(f32)


def _truncated(x):
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(f32)


def _ulp_up(x, i):
    """x with element i moved by one bf16 ulp"""
    x = x.copy()
    u = x.view(np.uint32)
    u[i] += np.uint32(0x10000)
    return x


class Fp32Sums:
    """reductions ACCUMULATED in float32, in the orders the engine's kernels use -- the restatement the head-room check is about"""

    @staticmethod
    def mm(a, b):
        """a . b as the matrix pipe accumulates it (v_mfma_f32_32x32x16_bf16): a k-step is 16 exact products summed and rounded
        to fp32 once; the k-steps' sums are added in fp32, four consecutive steps to one accumulator (a 64-k tile), the tiles'
        sums in a tree (split-K)"""
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        tiles = []
        for k0 in range(0, a.shape[1], 64):
            acc = np.zeros((a.shape[0], b.shape[1]), f32)
            for k in range(k0, min(k0 + 64, a.shape[1]), 16):
                acc = acc + a64[:, k:k + 16].dot(b64[k:k + 16]).astype(f32)
            tiles.append(acc)
        while len(tiles) > 1:
            tiles = [tiles[i] + tiles[i + 1] if i + 1 < len(tiles) else tiles[i] for i in range(0, len(tiles), 2)]
        return tiles[0]

    @staticmethod
    def colsum(x):
        """fp32 column sums by a reduction tree, as block reductions form them (numpy adds the ROWS of a C-ordered matrix one
        after the other; along the contiguous axis it sums in eight lanes, pairwise beyond 128 terms)"""
        return np.add.reduce(np.ascontiguousarray(x.T), axis=1, dtype=f32)

    @classmethod
    def stats(cls, z, eps, chunk=64):
        """fp32 batch mean and rstd as the engine forms them: a two-pass (mean, M2) per tile of `chunk` rows, the tiles merged
        after Chan et al. (the scheme of bn_stats_model, whose sums inside a tile run row after row)"""
        n, mean, m2 = f32(0), np.zeros(z.shape[1], f32), np.zeros(z.shape[1], f32)
        for r0 in range(0, z.shape[0], chunk):
            part = z[r0:r0 + chunk]
            nk = f32(part.shape[0])
            mk = cls.colsum(part) / nk
            d = part - mk
            tot = n + nk
            delta = mk - mean
            mean = mean + delta * (nk / tot)
            m2 = m2 + cls.colsum(d * d) + delta * delta * (n * nk / tot)
            n = tot
        return mean, f32(1) / np.sqrt(m2 / n + eps)


class ExactSums:
    """every reduction the float32 rounding of its exact value: the least round-off float32 storage allows, a lower envelope"""

    @staticmethod
    def mm(a, b):
        return a.astype(np.float64).dot(b.astype(np.float64)).astype(f32)

    @staticmethod
    def colsum(x):
        return x.astype(np.float64).sum(axis=0).astype(f32)

    @staticmethod
    def stats(z, eps):
        """the mean of the stored z, and rstd from the exact variance of the stored z about that stored mean"""
        z64 = z.astype(np.float64)
        mean = z64.mean(axis=0).astype(f32)
        var = ((z64 - mean.astype(np.float64)) ** 2).mean(axis=0)
        return mean, (1.0 / np.sqrt(var + float(eps))).astype(f32)


def _act32(u, kind):
    if kind == "relu":
        return np.maximum(u, f32(0))
    if kind == "sigmoid":
        return f32(1) / (f32(1) + np.exp(-u))
    if kind == "tanh":
        return np.tanh(u)
    return u


def _dact32(v, kind):
    if kind == "relu":
        return (v > 0).astype(f32)
    if kind == "sigmoid":
        return v * (f32(1) - v)
    if kind == "tanh":
        return f32(1) - v * v
    return np.ones_like(v)


def f32_step(net, X, criterion, masks=None, G0=None, mut=None, at=1, sums=Fp32Sums, ulp_at=None):
    """One training micro-batch of `net` (an OracleDNN: parameters and chain) in float32 with bf16 operand twins, in the engine's
    algebra; returns the taps bf16_links reads.  sums: how reductions are formed (Fp32Sums / ExactSums).  mut: one deliberate
    defect at hidden layer `at` (the mutation test); ulp_at: the element the "dz-ulp" defect moves (None: the largest)."""
    _mm32, _colsum, _stats32 = sums.mm, sums.colsum, sums.stats
    L, keep, eps = net.L, f32(net.keep), f32(net.bn_eps)
    W = [w.astype(f32) for w in net.W]
    b = [v.astype(f32) for v in net.b]
    Wb = [_twin(w) for w in W]
    X = np.ascontiguousarray(X, dtype=f32)
    n = f32(X.shape[0])
    tp = dict(X=X, Xb=_twin(X), z=[], mean=[], rstd=[], a=[], ab=[], masks=masks, Wb=Wb, dzb=[None] * L)
    xhat, vs, ss = [], [], []
    for l in range(L):
        inb = tp["Xb"] if l == 0 else tp["ab"][l - 1]
        z = _mm32(inb, Wb[l]) + b[l]
        if mut == "kstep" and l == at:  # one k-step of 16 missing from one 32 x 32 tile
            z[:32, :32] -= inb[:32, 16:32].dot(Wb[l][16:32, :32])
        u = z
        if net.bn:
            mean, rstd = _stats32(z, eps)
            d = z - mean
            xh = d * rstd
            u = xh if (mut == "nobeta" and l == at) else xh + net.beta[l].astype(f32)
            tp["mean"].append(mean)
            tp["rstd"].append(rstd)
            xhat.append(xh)
        v = _act32(u, net.nonlin)
        w = v
        if net.l2:
            s = (v * v).mean(axis=1, keepdims=True, dtype=f32)
            w = np.where(s > 1, v / s, v)
            ss.append(s)
        if net.dropout:
            w = w * masks[l].astype(f32) / keep
            if mut == "dropout2" and l == at:
                w = w / keep
        vs.append(v)
        tp["z"].append(z)
        tp["a"].append(w)
        tp["ab"].append(_truncated(w) if (mut == "truncate" and l == at) else _twin(w))
    tp["logits"] = _mm32(tp["ab"][L - 1], Wb[L]) + b[L]
    tp["dlogits"] = criterion(tp["logits"].astype(np.float64))[0].astype(f32)
    tp["dlogb"] = _twin(tp["dlogits"])
    G0 = G0 or {k: np.zeros(p.shape, f32) for k, p in net.params().items()}
    G = {k: g.copy() for k, g in G0.items()}
    G["W%d" % L] = G0["W%d" % L] + _mm32(tp["ab"][L - 1].T, tp["dlogb"])
    G["b%d" % L] = G0["b%d" % L] + _colsum(tp["dlogits"])
    up, w_up = tp["dlogb"], Wb[L]
    for l in range(L - 1, -1, -1):
        dw = _mm32(up, w_up.T)
        if net.dropout:
            dw = dw * masks[l].astype(f32) / keep
        if net.l2:
            v, s = vs[l], ss[l]
            dot = (dw * v).sum(axis=1, keepdims=True, dtype=f32)
            dw = np.where(s > 1, dw / s - v * (f32(2) * dot / (f32(H) * s * s)), dw)
            du = dw * _dact32(v, net.nonlin)
        else:
            du = dw * _dact32(tp["a"][l] * keep, net.nonlin)
        if net.bn:
            rows = n - f32(1) if (mut == "bn-rows" and l == at) else n
            m1 = _colsum(du) / rows
            m2 = _colsum(du * xhat[l]) / rows
            dz = tp["rstd"][l] * (du - m1 - xhat[l] * m2)
            G["beta%d" % l] = G0["beta%d" % l] + _colsum(du)
        else:
            dz = du
        dzb = _truncated(dz) if (mut == "dz-truncate" and l == at) else _twin(dz)
        if mut == "dz-ulp" and l == at:
            dzb = _ulp_up(dzb, ulp_at if ulp_at is not None else np.unravel_index(np.argmax(np.abs(dzb)), dzb.shape))
        tp["dzb"][l] = dzb
        inb = tp["Xb"] if l == 0 else tp["ab"][l - 1]
        G["W%d" % l] = G0["W%d" % l] + _mm32(inb.T, dzb)
        G["b%d" % l] = G0["b%d" % l] + _colsum(dz)
        up, w_up = dzb, Wb[l]
    assert all(g.dtype == f32 for g in G.values()) and tp["logits"].dtype == f32
    tp["G"], tp["G0"] = G, G0
    return tp


def _net(seed, chain, L):
    rng = np.random.default_rng(seed)
    net = OracleDNN(F_IN, L, H, O, gemm_dtype="bfloat16", **CHAINS[chain])
    randomize(net, rng)
    X = (rng.standard_normal((T, F_IN)) * 1.5).astype(f32)
    y = rng.integers(0, O, size=T)
    masks = [(rng.random((T, H)) < net.keep).astype(np.float64) for _ in range(L)] if net.dropout else None
    return net, X, y, masks


def _worst(ratios):
    name = max(ratios, key=ratios.get)
    return name, ratios[name]


def _fro(g, w):
    return float(np.linalg.norm(np.asarray(g, np.float64) - w) / max(np.linalg.norm(w), 1e-30))


CASCADE = dict(seed=5, chain="tanh", L=3)
# The two kinds of link whose bound, taken over from older tests as the issue of this file names them, an fp32-ACCUMULATING
# computation cannot use only a quarter of -- asserted at the bound itself, for the reasons written at
# test_every_link_leaves_headroom; every other link is asserted at HEADROOM
NO_QUARTER = ("F2", "B1 G[W")


def _scaled_ratios(net, taps, crit):
    """err / (HEADROOM x tol) of every link: at most 1 where the restatement uses no more than HEADROOM of the bound (link B2:
    its twin inside the rounding interval of want +- HEADROOM x tol)"""
    return link_ratios(*bf16_links(net, taps, crit, tol_scale=HEADROOM))


@pytest.mark.parametrize("sums", [Fp32Sums, ExactSums], ids=["fp32-sums", "exact-sums"])
def test_the_cascade_is_real_and_the_links_are_immune(sums):
    """tanh + batch norm, three layers, the CTC loss: the float32 restatement and the float64 oracle with bf16 operands -- two
    correct statements of the same step -- disagree on the parameter gradients by more than 1e-4 (W0 2.8e-3 with sums
    accumulated in fp32, 1.6e-3 even with every sum rounded once), yet every link of the restatement is inside its bound"""
    net, X, _, _ = _net(**CASCADE)
    crit = ctc_criterion(UTT, LABELS, LABEL_LEN)
    taps = f32_step(net, X, crit, sums=sums)
    z = net.forward_logits(X)
    dlog, _ = crit(z)
    net.backward_from_dlogits(dlog, 0.0, int(sum(LABEL_LEN)))
    fro = {k: _fro(taps["G"][k], net.G[k]) for k in net.G if k.startswith("W")}
    hidden = [_fro(taps["a"][l], net.last_cache[l]["a"]) for l in range(net.L)]
    name, worst = _worst(link_ratios(*bf16_links(net, taps, crit)))
    print("bf16-links cascade %-9s: whole-network gradients fro %s | hidden %s | worst link %s %.3f"
          % (sums.__name__, " ".join("%s %.1e" % kv for kv in sorted(fro.items())), " ".join("%.1e" % h for h in hidden), name, worst))
    assert max(fro.values()) > 1e-4, fro
    assert worst <= 1, (name, worst)


_sweeps = {}


def _sweep(chain, L, sums):
    """20 seeds of (chain, depth); every fourth under the CTC loss, the others under the cross-entropy; every fifth with a
    second micro-batch that accumulates onto the first one's sums.  {link: worst err / tol}, computed once."""
    key = (chain, L, sums)
    if key not in _sweeps:
        worst = {}
        for seed in range(20):
            net, X, y, masks = _net(100 + seed, chain, L)
            crit = ctc_criterion(UTT, LABELS, LABEL_LEN) if seed % 4 == 0 else xent_criterion(y)
            taps = f32_step(net, X, crit, masks, sums=sums)
            runs = [taps] + ([f32_step(net, X[::-1], crit, masks, G0=taps["G"], sums=sums)] if seed % 5 == 0 else [])
            for tp in runs:
                for k, r in _scaled_ratios(net, tp, crit).items():
                    worst[k] = max(worst.get(k, 0.0), HEADROOM * r)
        kinds = sorted({k.split()[0] + (" G[W]" if k.startswith("B1 G[W") else "") for k in worst})
        of = lambda k: k.split()[0] + (" G[W]" if k.startswith("B1 G[W") else "")
        print("bf16-links head-room %-9s %-10s L %d | err / tol: %s" % (sums.__name__, chain, L, " ".join(
            "%s %.3f" % (kind, max(r for k, r in worst.items() if of(k) == kind)) for kind in kinds)))
        _sweeps[key] = worst
    return _sweeps[key]


@pytest.mark.parametrize("L", [2, 4, 6])
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_every_link_leaves_headroom(chain, L):
    """The restatement that ACCUMULATES in float32 -- k-steps and tiles of the contractions, reduction trees, the tiled
    two-pass statistics -- uses at most HEADROOM of every tolerance bf16_links derives (B2, the sums, the loss, the twins) and
    of the activation and forward-contraction bounds (F1, F3, F4).  A derived tolerance that fails this is derived wrongly.

    Two kinds of link are taken over with their bound and cannot show a quarter; they are asserted at the bound, 1:
      F2 (statistics).  The bound is FOUR TIMES the error of an fp32 model of the same sums, at the better of two tile heights,
         its worst column (tests/test_gpu_dnn_edges.py: "the factor 4 covers a different but still correct summation
         order").  Another correct fp32 evaluation of those sums errs like the model itself, i.e. near a quarter by
         definition, and its worst column over a sweep lies above it: measured 0.30 .. 0.44 here, 0.20 .. 0.39 on the engine.
      B1 G[W] (the weight-gradient contraction, K = T = 143).  The bound allows 4e-7 = 6.7 x 2^-24 of sum |a b|.  An element
         passes one rounding per k-step sum, three additions inside a 64-k tile, two tree levels and the addition onto G:
         seven roundings of up to 2^-24 of a partial sum each, and the output layer's operands (a >= 0 behind a ReLU,
         dLogits > 0 off the label) do not cancel, so partial sums reach sum |a b|.  The worst case is 7 / 6.7 of the
         bound; the draws seen here reach 0.28 (the engine: 0.33).  At K = 64 (F1, F4: four roundings) the same count
         leaves 0.6 in the worst case and 0.25 is met.
    test_exactly_rounded_sums_leave_headroom holds the same bounds against the format alone."""
    worst = _sweep(chain, L, Fp32Sums)
    quarter = {k: r for k, r in worst.items() if not k.startswith(NO_QUARTER)}
    name, w = _worst(quarter)
    assert w <= HEADROOM, (name, w)
    name, w = _worst(worst)
    assert w <= 1, (name, w)


@pytest.mark.parametrize("L", [2, 4, 6])
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_exactly_rounded_sums_leave_headroom(chain, L):
    """the lower envelope: with every reduction the float32 rounding of its exact value, EVERY link -- F2 and B1 G[W] included
    -- stays within HEADROOM of its tolerance: each bound is at least four times what the float32 format itself costs"""
    name, w = _worst(_sweep(chain, L, ExactSums))
    assert w <= HEADROOM, (name, w)


MUTATIONS = [  # (defect, chain, the link that must fail)
    ("truncate", "tanh", "TW ab1"),       # a twin truncated where it should be rounded to nearest even
    ("dz-ulp", "tanh", "B2 dzb1"),        # the largest dz operand element moved by one bf16 ulp (see the test below for the others)
    ("kstep", "tanh", "F1 z1"),           # one k-step of 16 dropped from one contraction tile
    ("bn-rows", "tanh", "B2 dzb1"),       # BN backward means over T - 1 rows
    ("nobeta", "tanh", "F3 a1"),          # beta omitted
    ("dropout2", "relu-drop", "F3 a1"),   # a dropout scale applied twice
    ("dz-truncate", "tanh", "B2 dzb1"),   # the dz twin truncated: no fp32 dz is stored, the rounding interval must catch it
]


@pytest.mark.parametrize("mut,chain,expect", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_subtly_wrong_step_fails_a_link(mut, chain, expect):
    net, X, y, masks = _net(7, chain, 3)
    crit = xent_criterion(y)
    clean = link_ratios(*bf16_links(net, f32_step(net, X, crit, masks), crit))
    assert max(clean.values()) <= 1
    bad = link_ratios(*bf16_links(net, f32_step(net, X, crit, masks, mut=mut), crit))
    failed = sorted(k for k, r in bad.items() if r > 1)
    print("bf16-links mutation %-11s fails %s (err / tol %.3g)" % (mut, ", ".join(failed), bad[expect]))
    assert expect in failed, (mut, failed)


def test_which_dz_elements_a_one_ulp_move_is_caught_on():
    """The "dz-ulp" case above moves the LARGEST element, the favourable one.  B2 is an interval check -- there is no fp32 dz to
    compare the twin with -- so a one-ulp move passes on an element whose interval [round(want - tol), round(want + tol)] has
    two values and the move lands on the other one.  64 elements of layer 1 drawn at random: every element whose interval is
    ONE value must be caught, and those are the majority; the fraction caught is printed."""
    net, X, y, masks = _net(7, "tanh", 3)
    crit = xent_criterion(y)
    links, _ = bf16_links(net, f32_step(net, X, crit, masks), crit)
    tol = dict((name, t) for name, _, t in links)["B2 dzb1"]
    rng = np.random.default_rng(70)
    picks = [(int(r), int(c)) for r, c in zip(rng.integers(0, T, 64), rng.integers(0, H, 64))]
    caught, exact = 0, 0
    for at in picks:
        bad = link_ratios(*bf16_links(net, f32_step(net, X, crit, masks, mut="dz-ulp", ulp_at=at), crit))
        hit = bad["B2 dzb1"] > 1
        caught += hit
        exact += tol[at] == 0
        assert hit or tol[at] > 0, at
    print("bf16-links mutation dz-ulp on 64 random elements: %d caught, %d have a one-valued interval" % (caught, exact))
    assert exact > 32 and caught >= exact
