"""A reference MODEL of the batch-norm statistics, and the two conditions that make tests/test_gpu_dnn_edges.py's bound on
the device's mean / rstd meaningful.  No GPU here.

The engine computes a layer's column statistics in fp32 in two levels (tfkaldi_amd/csrc: the forward GEMM's EPI_COLSTATS
epilogue or bn_stats_partial_kernel give a two-pass (mean, M2) per chunk of rows; bn_act_forward_kernel /
bn_stats_final_kernel merge the chunks after Chan et al.).  `bn_stats_model` restates that in numpy float32 with the WORST
summation order such a scheme can have: within a chunk one running sum over the rows, the chunks merged one after the other.
The GPU test allows the device 4x this model's error against float64 on the same data (floored at one fp32 ulp), so:
  (i)  the model itself must be far inside the project's tolerance on the layer output (rtol 1e-4 + atol 2e-5,
       tests/test_gpu_engine_parity.py) -- a quarter of it -- and below 1e-5 relative on rstd: 4x the model is then still a bound
       that a correct kernel's consumers cannot feel;
  (ii) a ONE-pass E[z^2] - E[z]^2 in fp32 must miss rstd by more than 1e-4 relative on the offset data (|mean| = 30, spread 1):
       the data separates a cancelling formula from a two-pass one by a factor the bound cannot hide.

How (i) is measured.  The normalised value xhat = (z - mean) * rstd has a column spread of one by construction, and the
tolerance on a value of one is 1e-4 + 2e-5 = 1.2e-4: the model's xhat must stay within a quarter of that, 3e-5, on every element.
The same tolerance taken element by element -- 2e-5 alone where xhat is near zero -- is printed as well but cannot be asked of ANY
fp32 statistic on this data: at T = 2 the mean of two values near 30 is known to half an ulp of 30 (9.5e-7) at best, and a column
whose two values nearly agree has rstd = 31.6, which turns that half ulp into 3e-5 of xhat.  Measured (offset 30, chunks of 64 /
128 rows): element-wise 0.44 / 0.83 / 0.27 / 0.44 of the tolerance at T = 2 / 129 / 2177 / 4225 (the running sum of 128 values
near 30 is off by ~1e-5 after the division), against 0.03 and less on ordinary data.  No smaller offset helps: the model's
error falls linearly with offset / spread and the one-pass error of (ii) with its square -- at an offset of 9 the first is 0.26
and the second has already dropped to 9e-5 at T = 129.

How (ii) is measured: on the WORST offset column.  Which way the roundings of the two running sums fall is chance per column
(the best column of 64 is within 5e-7 .. 5e-6 at every T); a kernel is judged on all of its columns."""
import numpy as np
import pytest

from oracle.dnn_oracle import BN_EPS, _running_sum, bn_stats_model, stats64  # noqa: F401 (the model lives with the oracle: the link checker bounds with it too)

OFFSET, F, H = 30.0, 20, 130
CONSTANT_COL = 128                # first column of the second 128-column block
ROWS = [2, 129, 2177, 4225]


def offset_layer(rng, d_in, d_out, x_std, constant_col=None):
    """(W, b) of a layer whose affine output has |mean| = OFFSET on every other column and a column spread of about 1 for
    inputs of standard deviation x_std; column `constant_col` has zero weights: its output is the bias, bit for bit"""
    W = (rng.standard_normal((d_in, d_out)) / (np.sqrt(d_in) * x_std)).astype(np.float32)
    b = (rng.standard_normal(d_out) * 0.1).astype(np.float32)
    b[::2] = OFFSET
    if constant_col is not None:
        W[:, constant_col] = 0.0
    return W, b


def one_pass_rstd(z):
    """rstd from E[z^2] - E[z]^2 with fp32 running sums: what the statistics must NOT be"""
    z = np.ascontiguousarray(z, dtype=np.float32)
    f = np.float32
    T = f(z.shape[0])
    mean = _running_sum(z) / T
    var = np.maximum(_running_sum(z * z) / T - mean * mean, f(0))
    return f(1) / np.sqrt(var + f(BN_EPS))


def _data(T, offset):
    rng = np.random.default_rng(900 + T)
    X = (rng.standard_normal((T, F)) * 1.5).astype(np.float32)
    if offset:
        W, b = offset_layer(rng, F, H, 1.5, constant_col=CONSTANT_COL)
    else:
        W = (rng.standard_normal((F, H)) / np.sqrt(F)).astype(np.float32)
        b = (rng.standard_normal(H) * 0.1).astype(np.float32)
    return (X.astype(np.float64).dot(W.astype(np.float64)) + b).astype(np.float32)


@pytest.mark.parametrize("offset", [False, True], ids=["ordinary", "offset"])
@pytest.mark.parametrize("T", ROWS)
def test_model_is_far_inside_the_output_tolerance_and_one_pass_is_not(T, offset):
    z = _data(T, offset)
    mean, var, rstd = stats64(z)
    xhat = (z - mean) * rstd
    worst = {}
    for c in (64, 128):
        m, _, r = bn_stats_model(z, c)
        d = np.abs((z.astype(np.float64) - m) * r - xhat)
        worst[c] = (float(np.abs(m - mean).max()), float((np.abs(r - rstd) / rstd).max()), float(d.max()),
                    float((d / (1e-4 * np.abs(xhat) + 2e-5)).max()))
    naive = np.abs(one_pass_rstd(z) - rstd) / rstd
    live = np.ones(H, dtype=bool)
    if offset:
        live = np.abs(mean) > OFFSET / 2
        live[CONSTANT_COL] = False  # (variance 0: judged separately below)
    print("bn-stats-model T %4d %-8s | model: mean %.1e rstd %.1e xhat %.1e (element-wise %.2f of the tolerance) | "
          "one-pass rstd: %.1e .. %.1e" % ((T, "offset" if offset else "ordinary") + tuple(max(w[i] for w in worst.values())
                                                                                       for i in range(4))
                                           + (naive[live].min(), naive[live].max())))
    for c, (_, r_err, x_err, _) in worst.items():
        assert x_err <= 0.25 * (1e-4 + 2e-5), (c, x_err)   # (i)
        assert r_err < 1e-5, (c, r_err)
    if offset:
        for c in (64, 128):  # the constant column: M2 is exactly 0 in the model as in float64
            _, v, r = bn_stats_model(z, c)
            assert v[CONSTANT_COL] == 0 and var[CONSTANT_COL] == 0
            np.testing.assert_allclose(r[CONSTANT_COL], 1 / np.sqrt(BN_EPS), rtol=1e-6)
        assert naive[live].max() > 1e-4, naive[live].max()  # (ii)
