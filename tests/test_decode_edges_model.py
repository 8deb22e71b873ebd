"""The bound that tests/test_gpu_decode_edges.py puts on softmax_rows_kernel's log(posterior / prior), and a float32 numpy
RESTATEMENT of the kernel's formula that has to stay within half of it.  No GPU here: the logits are synthetic, with the spreads
of the GPU test's two regimes.

The kernel (tfkaldi_amd/csrc/kernels.hip) computes, per row of fp32 logits z and with every operation rounded to fp32,
    mx = max z;  se = sum expf(z - mx);  lse = mx + logf(se);  out[c] = (z[c] - lse) - logf(prior[c]).
The reference is want = (z - L) - log(float64(prior)) with L the float64 log-sum-exp of the same z.  With u = 2^-24 (half an
fp32 ulp of one) and every library function within one ulp (2u relative):
  * se: each term carries expf's ulp (2u) and the rounding of its argument, u |z - mx| relative; weighted by the posteriors
    that is u * sum p (mx - z) <= u * (L - sum p z) = u * entropy <= u log O.  The additions: at most 4 NV (register kernels) or
    ceil(O / 256) (generic kernel) sequential ones per thread, 6 wave shuffles, 3 wave sums.  delta_se <= u (2 + log O + depth).
  * logf(se): delta_se from its argument plus its own ulp, 2u log se <= 2u log O  (1 <= se <= O).
  * mx + logf(se): half an ulp of the sum, u |lse|.
  * z - lse: u |z - lse|.      * logf(prior): 2u |log prior|.      * the last subtraction: u |want|.
  total <= u (|L| + |z - L| + 2 |log prior| + |want|) + u (2 + 3 log O + depth)
The test uses 2^-23 (|z - L| + |L| + |log prior| + |want|) + CONST(O), CONST(O) = 2^-24 (2 + 3 log O + depth(O)): the first
term is the sum above with u doubled on three of its four parts (room for a library function at two ulp), never less than it.
CONST is 1.1e-6 at O = 3 and 4.4e-6 at O = 8193.  Where that is looser than the suite's earlier rule for this output
(tests/test_gpu_eval_fused.py: 2e-5 + 2e-5 |want|) -- a |want| near zero made of large parts -- the earlier rule holds: the
bound is the smaller of the two at every element.

Two conditions make the bound meaningful, both asserted here: the restatement stays within HALF of it on every element
(a correct fp32 evaluation has room), and the bound is far below what a wrong kernel does -- a prior read one column off moves
an element by |log p[c] - log p[c + 1]|, O(1); a tail column that enters the sum changes lse by O(1 / O) or more.

Posteriors: rtol 2e-5 (the suite's) plus 8 spacings of the fp32 denormals, 2^-146, instead of the earlier atol 1e-9: expf's
result and its product with 1 / se are each rounded to the denormal grid (half a spacing each) where the posterior is below
2^-126, on top of the relative terms."""
import numpy as np
import pytest

T = 19
WIDTHS = [3, 1021, 1024, 1025, 2048, 2049, 4094, 4097, 8192, 8193]
POST_RTOL, POST_ATOL = 2e-5, 2.0 ** -146
TINY = float(np.finfo(np.float32).tiny)  # the smallest normal fp32
PRIOR_EDGES = (1e-30, TINY, 1.0)


def sum_depth(O):
    """additions on the longest path of the kernel's row sum"""
    nc4 = (O + 3) // 4
    per_thread = 4 * next((nv for nv in (1, 2, 4, 8) if nc4 <= 256 * nv), 0) or -(-O // 256)
    return per_thread + 6 + 3


def log_prior_const(O):
    return 2.0 ** -24 * (2 + 3 * np.log(O) + sum_depth(O))


def lse64(z):
    z = np.asarray(z, dtype=np.float64)
    mx = z.max(axis=1, keepdims=True)
    return mx + np.log(np.exp(z - mx).sum(axis=1, keepdims=True))


def softmax64(z):
    return np.exp(np.asarray(z, dtype=np.float64) - lse64(z))


def log_prior_reference(z, prior):
    """(want, bound) of log(posterior / prior) for fp32 logits z [T, O] and an fp32 prior [O] (positive entries)"""
    z64, L = np.asarray(z, dtype=np.float64), lse64(z)
    with np.errstate(divide="ignore"):
        lp = np.log(np.asarray(prior, dtype=np.float32).astype(np.float64))
    want = (z64 - L) - lp
    with np.errstate(invalid="ignore"):
        derived = 2.0 ** -23 * (np.abs(z64 - L) + np.abs(L) + np.abs(lp) + np.abs(want)) + log_prior_const(z64.shape[1])
        bound = np.minimum(derived, 2e-5 + 2e-5 * np.abs(want))
    return want, bound


def rows_f32(z, prior=None):
    """softmax_rows_kernel restated in numpy float32: posteriors, or log(posterior / prior) with a prior"""
    f = np.float32
    z = np.ascontiguousarray(z, dtype=f)
    mx = z.max(axis=1, keepdims=True)
    ex = np.exp(z - mx)
    se = ex.sum(axis=1, keepdims=True, dtype=f)
    assert ex.dtype == se.dtype == f
    if prior is None:
        return ex * (f(1) / se)
    lse = mx + np.log(se)
    with np.errstate(divide="ignore"):
        out = (z - lse) - np.log(np.ascontiguousarray(prior, dtype=f))
    assert out.dtype == f
    return out


def random_prior(rng, O):
    p = rng.random(O) + 0.05
    return (p / p.sum()).astype(np.float32)


def edge_prior(rng, O, shift):
    """a random prior with 1e-30, the smallest normal fp32 and exactly 1.0 in column 0, column O - 1 and every slot of the last
    live float4, the three values rotated by `shift` so that three priors put each value in each place"""
    p = random_prior(rng, O)
    cols = sorted(set([0] + list(range(4 * ((O - 1) // 4), O))))
    for i, c in enumerate(cols):
        p[c] = PRIOR_EDGES[(i + shift) % 3]
    return p


def synthetic_logits(rng, O, spread):
    """[T, O] fp32 logits whose rows span `spread` .. 1.5 `spread` around an offset of a few units -- the magnitudes the GPU
    test's net produces (it picks frames of similar spread: a row of logits near 600 has an fp32 ulp of 6e-5, which no fp32
    evaluation of lse can keep inside the earlier rule's 2e-5 where |want| is small)"""
    z = rng.standard_normal((T, O))
    z -= 0.5 * (z.max(axis=1, keepdims=True) + z.min(axis=1, keepdims=True))
    z *= spread * rng.uniform(1.0, 1.5, size=(T, 1)) / (z.max(axis=1, keepdims=True) - z.min(axis=1, keepdims=True))
    return (z + rng.standard_normal((T, 1)) * 3).astype(np.float32)


def worst_ratio(got, want, bound):
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(np.abs(np.asarray(got, dtype=np.float64) - want) / bound))


@pytest.mark.parametrize("regime,spread", [("initial", 8.0), ("peaked", 140.0)])
@pytest.mark.parametrize("O", WIDTHS)
def test_f32_restatement_is_within_half_the_bound(O, regime, spread):
    rng = np.random.default_rng(O)
    z = synthetic_logits(rng, O, spread)
    if regime == "peaked":
        assert ((z - z.max(axis=1, keepdims=True)) < -104.5).any()
    figures = []
    for prior in [random_prior(rng, O)] + [edge_prior(rng, O, k) for k in range(3)]:
        want, bound = log_prior_reference(z, prior)
        got = rows_f32(z, prior)
        assert np.isfinite(got).all() and np.isfinite(want).all()
        assert (bound <= 2e-5 + 2e-5 * np.abs(want)).all()  # never looser than the earlier rule
        figures.append(worst_ratio(got, want, bound))
        assert figures[-1] <= 0.5, figures
        # what the bound must catch: the prior read one column off
        if O > 3:
            off = rows_f32(z, np.roll(prior, 1))
            assert (np.abs(off - want) > bound).mean() > 0.9
    post, want = rows_f32(z), softmax64(z)
    err = np.abs(post - want)
    ratio = float((err / (POST_RTOL * want + POST_ATOL)).max())
    print("decode-edges-model O %4d %-7s | log(post / prior): restatement / bound %s | posteriors: restatement / tolerance %.2f"
          % (O, regime, " ".join("%.2f" % r for r in figures), ratio))
    assert ratio <= 0.5, ratio
    under = (z - z.max(axis=1, keepdims=True)) < -104.5
    assert (post[under] == 0).all() and (post >= 0).all()


def test_zero_prior_gives_plus_infinity():
    rng = np.random.default_rng(0)
    z = synthetic_logits(rng, 9, 8.0)
    prior = random_prior(rng, 9)
    prior[[0, 8]] = 0.0
    got = rows_f32(z, prior)
    assert np.isposinf(got[:, [0, 8]]).all() and np.isfinite(got[:, 1:8]).all()
