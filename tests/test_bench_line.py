"""bench.py's plain run and its --dump-outputs: the contract's line from the timed steps alone, and the arrays those steps
computed written as small float .npy files that are the same from run to run (CPU: the helpers on a stand-in engine; GPU: the
command itself)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from tfkaldi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "host_fed_value", "kernel_ms_per_step", "sustained", "exchange_model", "cpu_baseline", "decode", "eval",
             "exact_fp32", "api_fed_value")


class _StandInEngine(object):
    """Engine.get for the shapes of one Workload; values from a seeded generator"""

    def __init__(self, w, seed):
        self.w, self.seed = w, seed

    def get(self, kind, layer):
        w = self.w
        if kind == _lib.WEIGHTS:
            shape = (bench.F if layer == 0 else w.H, w.O if layer == w.L else w.H)
        elif kind == _lib.BIASES:
            shape = (w.O if layer == w.L else w.H,)
        else:
            shape = (w.H,)
        rng = np.random.default_rng((self.seed, kind, layer))
        return rng.standard_normal(shape, dtype=np.float32)


@pytest.mark.parametrize("config", ["cfg2", "cfg4"])
def test_dump_outputs_are_small_seeded_floats(tmp_path, config):
    w = bench.Workload(config)
    losses = [7.6, 7.5, 7.25]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), w, _StandInEngine(w, 5), losses)
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(os.listdir(str(tmp_path / "b")))
    assert len(names) == 2 + 2 * (w.L + 1) + 3 * w.L
    total = 0
    for name in names:
        a, b = np.load(str(tmp_path / "a" / name)), np.load(str(tmp_path / "b" / name))
        assert a.dtype in (np.float32, np.float64), name
        np.testing.assert_array_equal(a, b, err_msg=name)  # the same sample of the same parameters: the same file
        total += os.path.getsize(str(tmp_path / "a" / name))
    assert total <= 64 << 20
    assert np.load(str(tmp_path / "a" / "loss.npy")).tolist() == [7.25]
    assert np.load(str(tmp_path / "a" / "losses.npy")).tolist() == losses
    full = _StandInEngine(w, 5).get(_lib.WEIGHTS, w.L).ravel()
    sample = np.load(str(tmp_path / "a" / ("weights_%d.npy" % w.L)))
    assert sample.size == min(full.size, bench.DUMP_SAMPLE) and np.isin(sample, full).all()
    # other parameters, other files
    bench.dump_outputs(str(tmp_path / "c"), w, _StandInEngine(w, 6), losses)
    assert not np.array_equal(sample, np.load(str(tmp_path / "c" / ("weights_%d.npy" % w.L))))


def test_contract_line_says_what_was_timed():
    w = bench.Workload("cfg2")
    args = argparse.Namespace(steps=20, warmup=5, dtype=w.dtype)
    line = bench.contract_line(w, args, 2, 16, 0.05, [2.4, 2.5], "nccl", {"loss_first_last": [7.6, 7.0]})
    assert all(k in line for k in CONTRACT)
    assert line["ms_per_step"] == pytest.approx(2.5) and line["value"] == pytest.approx(2 * 1024 * 20 / 0.05)
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["n_gpus"] == 2 and line["rccl_ranks"] == 2
    assert line["config"]["global_frames"] == 2048 and line["loss_first_last"] == [7.6, 7.0]
    json.dumps(line)


def test_bench_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_is_lean_and_dumps_the_same_outputs(gpu, tmp_path):
    """`bench.py --gpus 1 --steps 4 --warmup 2 --dump-outputs DIR`, twice: the contract's line without any diagnostic leg,
    `steps` timed steps, and the last step's loss and parameters in DIR -- the same inputs, so the same outputs"""
    lines = []
    for d in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                              "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=280)
        assert out.returncode == 0, out.stderr[-3000:]
        stdout = out.stdout.strip().splitlines()
        assert len(stdout) == 1, out.stdout[-2000:]
        lines.append(json.loads(stdout[0]))
    line = lines[0]
    assert all(k in line for k in CONTRACT) and not [k for k in FULL_ONLY if k in line], sorted(line)
    assert line["steps"] == 4 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1024 * 1e3 / line["ms_per_step"])
    assert abs(line["loss_first_last"][0] - np.log(2000)) < 1e-3
    losses = np.load(str(tmp_path / "a" / "losses.npy"))
    assert losses.tolist() == line["loss_trace_gpu"] and losses[-1] == line["loss_first_last"][1]
    assert np.load(str(tmp_path / "a" / "loss.npy")).tolist() == [line["loss_first_last"][1]]
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(os.listdir(str(tmp_path / "b"))) and len(names) == 2 + 2 * 7 + 3 * 6
    for name in names:
        a, b = np.load(str(tmp_path / "a" / name)), np.load(str(tmp_path / "b" / name))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7, err_msg=name)
