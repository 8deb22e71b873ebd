"""The RCCL call path on the one GPU of the test box.  (1) A single-rank "nccl" process group (TFK_FORCE_DP=1) drives
DataParallel.train_step / eval_step exactly as a multi-GPU job does -- torch-owned engine state, bucket callback
-> async all-reduce on RCCL's stream -> wait on the engine stream -> apply -- and must reproduce the plain
single-process run bit for bit (a 1-rank SUM all-reduce is the identity).  bench.py's N>1 branch is run the same
way.  (2) SEVERAL real RCCL ranks: one per GPU when the box has them, else all on GPU 0 with a host name each
(TFK_FAKE_NODES -> NCCL_HOSTID: RCCL's duplicate-device check compares host hash + bus id), the collectives going
through RCCL's socket transport -- the exchange options against the serial run, `bench.py --gpus N`, `Nnet.train`
under torchrun, the CTC loss."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_dp_two_ranks import _collect, _data, _engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def _worker(rank, port, num_mb, out_dir, mode="sharded", comm="native", dtype="float32"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      TFK_FORCE_DP="1", HSA_ENABLE_IPC_MODE_LEGACY="0", TFK_DP_MIN_SHARD="64",
                      TFK_DP_COMM="native" if comm == "unloadable" else comm)
    if comm == "unloadable":  # the library cannot bind RCCL: every rank agrees to run the exchange through torch.distributed
        os.environ["TFK_RCCL_LIB"] = "/nonexistent/librccl.so"
    planes = comm == "native+planes"  # the direct algorithm (grouped send / recv: none with one rank) + twin rows gathered
    if planes:
        os.environ.update(TFK_DP_COMM="native", TFK_DP_ALGO="direct", TFK_DP_GATHER="planes")
        comm = "native"
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from tfkaldi_amd.dataparallel import DataParallel, init_from_env
    init_from_env()
    assert dist.get_backend() == "nccl"
    dp = DataParallel(mode=mode)
    assert dp.enabled
    eng = _engine(torch_state=True, dtype=dtype)
    losses = [dp.train_step(eng, _data(num_mb, step)) for step in range(3)]
    # who launched the collectives: the library itself (csrc/exchange.hip) or BucketReducer through torch.distributed
    assert dp.reducer(eng).native == (comm == "native")
    assert (dp.native_failure is not None) == (comm == "unloadable"), dp.native_failure
    if comm == "unloadable":
        assert "could not be loaded" in dp.reducer(eng).fallback_reason
    if mode == "sharded":  # RCCL's reduce-scatter / all-gather really carried the step
        assert "rs" in dp.last_kinds, dp.last_kinds
        assert any("reduce_scatter" in name for name in dp.last_executed), dp.last_executed
        assert any("all_gather" in name for name in dp.last_executed), dp.last_executed
    losses.append(dp.eval_step(eng, _data(num_mb, 9)))
    if planes and mode == "sharded":
        red = dp.reducer(eng)
        assert red.planes and red.masters_stale and red.exchange_info()["reduce_scatter"] == "direct"
        assert any("three-plane twins" in name for name in dp.last_executed), dp.last_executed
    dp.gather_parameters(eng)
    np.savez(os.path.join(out_dir, "rccl.npz"), **_collect(eng, losses))
    eng.close()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("comm,dtype", [("native", "float32"), ("torch", "float32"), ("unloadable", "float32"),
                                        ("native", "float32x3"), ("torch", "float32x3"), ("native+planes", "float32x3")])
@pytest.mark.parametrize("mode", ["sharded", "allreduce"])
def test_single_rank_rccl_is_identity(gpu, tmp_path, mode, comm, dtype):
    """(float32x3: the exchange gathers fp32 parameters and the engine rebuilds its three-plane twins from them -- with one
    rank that must be the identity too, bit for bit)"""
    import torch.multiprocessing as mp
    num_mb = 3
    mp.spawn(_worker, args=(_free_port(), num_mb, str(tmp_path), mode, comm, dtype), nprocs=1, join=True)
    eng = _engine(torch_state=False, dtype=dtype)
    want = []
    for step in range(3):
        mbs = _data(num_mb, step)
        for i, (X, y) in enumerate(mbs):
            eng.accumulate(X, y, last=(i == len(mbs) - 1))
        want.append(eng.apply())
    # the validation pass as DataParallel.eval_step runs it (plain micro-batches as ONE stacked pass: the frames' losses are
    # summed in one reduction, which rounds differently from three sums added up -- bit-for-bit needs the same order)
    from tfkaldi_amd.dataparallel import _eval_accumulate_all
    _eval_accumulate_all(eng, _data(num_mb, 9))
    want.append(eng.eval_finish())
    ref = _collect(eng, want)
    eng.close()
    got = np.load(os.path.join(str(tmp_path), "rccl.npz"))
    for k, v in ref.items():
        np.testing.assert_array_equal(got[k], v, err_msg=k)


@pytest.mark.timeout(600)
def test_bench_dp_branch_over_rccl(gpu):
    """bench.py's N>1 code path (callback all-reduce + barrier + MAX over ranks) with one RCCL rank"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0", TFK_FORCE_DP="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup",
                          "2", "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["value"] > 0
    assert abs(line["loss_first_last"][0] - np.log(2000)) < 1e-3
    assert line["rccl_ranks"] == 1 and line["dist_backend"] == "nccl" and line["exchange"] == "sharded"
    # what RAN: RCCL's own reduce-scatter / all-gather on views of the engine state, the 32 MiB coalescing of cfg2's spans
    assert line["exchange_driver"].startswith("library"), line["exchange_driver"]
    assert line["collectives_last_step"].count("rccl:reduce_scatter") == 3, line["collectives_last_step"]
    assert line["collectives_last_step"].count("rccl:all_gather") == 3
    assert line["collectives_last_step"].count("rccl:all_reduce") == 2
    assert [n for _, n in line["collective_spans_last_step"] if n > 1 << 20] == [12484608, 8388608, 5095424]
    assert line["host_fed_value"] > 0 and len(line["loss_trace_gpu"]) == 7
    # the self-diagnosing part of an N > 1 line: what is in force, the algorithm x wire A/B, the per-phase device times per rank
    assert line["exchange_algorithm"] == {"reduce_scatter": "rccl", "all_gather": "rccl", "wire": "fp32", "chosen_by": "default",
                                          "gather": "fp32 parameters"}
    ab = line["exchange_ab"]["ms_per_step"]
    assert sorted(ab) == ["auto/fp32", "direct/bf16", "direct/fp32", "direct/fp32+planes", "rccl/bf16", "rccl/fp32",
                          "rccl/fp32+planes"] and all(0.5 < v < 50 for v in ab.values()), ab
    spans = line["exchange_ab"]["ms_per_step_by_span_MiB"]
    assert sorted(spans, key=int) == ["16", "32", "64", "128"] and all(0.5 < v < 50 for v in spans.values()), spans
    assert line["exchange_ab"]["auto"]["chosen_by"] == "tuned at attach" and "tuned_us_slowest_rank" in line["exchange_ab"]["auto"]
    assert line["exchange_phases"]["exchange"]["reduce_scatter"] == "rccl"  # back to what `value` ran with
    ph = line["exchange_phases"]["per_rank"]
    assert sorted(ph) == sorted(["reduce_scatter", "all_reduce", "tail_exposed", "adam", "all_gather", "twin_rebuild", "gather_exposed"])
    assert all(len(v) == 1 and v[0] >= 0 for v in ph.values()) and ph["adam"][0] > 0 and ph["reduce_scatter"][0] > 0, ph
    print("exchange A/B (one RCCL rank):", ab)
    print("exchange phases (one RCCL rank):", {k: round(v[0], 4) for k, v in ph.items()})
    sus = line["sustained"]
    assert sus["seconds"] >= 3.0 and sus["value"] > 0 and 0.8 < sus["value_over_sustained"] < 1.5, sus
    assert sus["samples"] >= 3 and sus["socket_power_w_mean"] > 100 and sus["shader_clock_mhz_mean"] > 500, sus


@pytest.mark.timeout(600)
def test_bench_line_survives_stuck_diagnostics(gpu):
    """bench.py at N > 1 measures the contract's fields first and runs its diagnostic legs (sustained leg, exchange A/B, phase
    times, Nnet.train) behind them under a watchdog: with a budget those legs cannot meet, rank 0 still prints ONE line with the
    contract's fields and `incomplete`, and the process leaves with status 0 (a rank stuck in a collective cannot be joined)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0", TFK_FORCE_DP="1", HSA_ENABLE_IPC_MODE_LEGACY="0", TFK_BENCH_DIAG_BUDGET_S="1.0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup",
                          "2", "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert "incomplete" in line and line["value"] > 0 and line["n_gpus"] == 1 and line["ms_per_step"] > 0
    assert line["config"]["name"] == "cfg2" and line["scaling"] == "weak" and "sustained" not in line


@pytest.mark.timeout(600)
def test_bench_self_launches_its_ranks(gpu):
    """`python bench.py --gpus 2` from a bare environment (no WORLD_SIZE): bench.py starts its own ranks through
    torch.distributed.run.  On the 1-GPU test box the two ranks share the device and talk over gloo (the torch.distributed
    driver; test_bench_over_real_rccl_ranks is the RCCL run); with >= 2 GPUs this is the driver's RCCL command as it stands."""
    import torch
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    real = torch.cuda.device_count() >= 2
    if not real:
        env.update(TFK_SHARE_DEVICE="1", TFK_DIST_BACKEND="gloo")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup",
                          "2"], env=env, capture_output=True, text=True, timeout=550)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["value"] > 0 and len(line["per_rank_ms_per_step"]) == 2
    assert line["config"]["global_frames"] == 2048 and line["scaling"] == "weak"
    assert line["rccl_ranks"] == (2 if real else 0) and line["dist_backend"] == ("nccl" if real else "gloo")
    assert abs(line["loss_first_last"][0] - np.log(2000)) < 1e-3
    if not real:  # the line says what really ran: the sharded protocol when this gloo build can reduce-scatter device
        # tensors (the reducer probes it), else all-reduce + replicated optimiser
        assert line["exchange_requested"] == "sharded"
        if line["exchange"] == "sharded":
            assert "reduce_scatter_tensor" in line["collectives_last_step"]
        else:
            assert line["exchange"] == "allreduce" and set(line["collectives_last_step"]) == {"all_reduce"}


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("world,config", [(2, "cfg2"), (4, "cfg2"), (2, "cfg3"), (2, "cfg4"), (8, "cfg2")])
def test_bench_over_real_rccl_ranks(gpu, world, config):
    """the driver's `bench.py --gpus N` with N REAL RCCL ranks (one per GPU, or all on GPU 0 claiming a host each: the transport
    is then RCCL's socket path and the rates mean nothing): the contract's line from the in-library exchange, and the whole
    self-diagnosis behind it -- exchange_ab over every algorithm x wire x gather x span size and the library's tuning pass,
    per-phase device times per rank, the sustained leg, Nnet.train under N ranks -- inside its budget (`incomplete` absent)."""
    import torch
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    if torch.cuda.device_count() < world:
        env["TFK_FAKE_NODES"] = "1"
    # (eight ranks on one GPU through sockets: ~0.3 s per step -- the diagnostics need more than the 300 s they get on a real node)
    env.update(TFK_BENCH_SUSTAIN_S="1", TFK_BENCH_PREWARM_MS="0", TFK_BENCH_DIAG_BUDGET_S="900")
    if world == 8:  # (Nnet.train under real ranks: the 2- and 4-rank cases)
        env.update(TFK_BENCH_AB_STEPS="3", TFK_BENCH_SUSTAIN_MIN_STEPS="10", TFK_BENCH_API_FED="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "4", "--warmup", "2",
                          "--full", "--config", config], env=env, capture_output=True, text=True, timeout=1100)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert "incomplete" not in line, line["incomplete"]
    assert line["n_gpus"] == world and line["rccl_ranks"] == world and line["dist_backend"] == "nccl"
    assert line["value"] > 0 and len(line["per_rank_ms_per_step"]) == world and line["scaling"] == "weak"
    assert line["config"]["name"] == config and line["config"]["global_frames"] == world * line["config"]["frames_per_gpu"]
    assert line["exchange"] == "sharded" and line["exchange_driver"].startswith("library (csrc/exchange.hip, rccl)")
    assert any("reduce_scatter" in c for c in line["collectives_last_step"])
    assert any("all_gather" in c for c in line["collectives_last_step"])
    assert abs(line["loss_first_last"][0] - np.log({"cfg2": 2000, "cfg3": 4000, "cfg4": 8000}[config])) < 1e-3
    ab = line["exchange_ab"]
    want = {"rccl/fp32", "rccl/bf16", "direct/fp32", "direct/bf16", "auto/fp32"}
    if config == "cfg2":
        want |= {"rccl/fp32+planes", "direct/fp32+planes"}
    assert want <= set(ab["ms_per_step"]) and all(v > 0 for v in ab["ms_per_step"].values()), ab
    assert set(ab["ms_per_step_by_span_MiB"]) == {"16", "32", "64", "128"}
    assert set(ab["auto"]["tuned_us_slowest_rank"]) == {"reduce_scatter_rccl", "reduce_scatter_direct", "all_gather_rccl",
                                                        "all_gather_direct"}
    ph = line["exchange_phases"]
    assert ph["steps"] == 10 and all(len(v) == world for v in ph["per_rank"].values())
    assert all(x > 0 for x in ph["per_rank"]["reduce_scatter"] + ph["per_rank"]["all_gather"] + ph["per_rank"]["adam"])
    # the rate the wire ran at (to hold against exchange_model's link rates): one figure per rank and phase
    rate = ph["measured_wire_rate"]
    for phase in ("reduce_scatter", "all_gather"):
        assert len(rate[phase]["GB_per_s_per_rank"]) == world and rate[phase]["slowest_rank_GB_per_s"] > 0, rate
    assert line["sustained"]["value"] > 0
    if world < 8:
        assert line["api_fed_value"] > 0, line.get("api_fed_error")
    assert line["exchange_model"]["per_world"][str(world)]["predicted_ms_per_step_direct"] > 0
    print("bench --gpus %d %s over real RCCL: exchange_ab %s" % (world, config, ab["ms_per_step"]))


@pytest.mark.timeout(1200)
def test_bench_eight_ranks_dry_run(gpu):
    """the driver's `bench.py --gpus 8` on one GPU: eight ranks share the device over gloo (TFK_SHARE_DEVICE), the
    sharded protocol runs with the reduce-scatter emulated -- every code path of the 8-rank bench line executes: the
    self-launch, the per-rank batches, the n / 8 shards of cfg2's spans, barrier + MAX over ranks, the report"""
    import torch
    if torch.cuda.device_count() >= 8:
        pytest.skip("a real 8-GPU node runs the real thing (test_bench_self_launches_its_ranks covers the launcher)")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(TFK_SHARE_DEVICE="1", TFK_DIST_BACKEND="gloo", TFK_DP_EMULATE_RS="1", TFK_BENCH_PREWARM_MS="0",
               OMP_NUM_THREADS="2", TFK_BENCH_SUSTAIN_S="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup",
                          "2", "--full"], env=env, capture_output=True, text=True, timeout=1100)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 8 and line["value"] > 0 and len(line["per_rank_ms_per_step"]) == 8
    assert line["config"]["global_frames"] == 8192 and line["scaling"] == "weak"
    assert line["exchange"] == "sharded"
    assert ("reduce_scatter_tensor" in line["collectives_last_step"]
            or "all_reduce(emulating reduce_scatter)" in line["collectives_last_step"])
    assert any(c.startswith("all_gather") for c in line["collectives_last_step"])
    assert all(n % 32 == 0 for _, n in line["collective_spans_last_step"][1:5])
    assert abs(line["loss_first_last"][0] - np.log(2000)) < 1e-3
    # the A/B block of an N > 1 line: over gloo the exchange runs through torch.distributed, which has one algorithm -- said so
    print("exchange_ab (8 gloo ranks on one GPU):", line["exchange_ab"])
    assert "torch.distributed/fp32" in line["exchange_ab"]["ms_per_step"] and "unavailable" in line["exchange_ab"]


def _rccl_worker(rank, world, port, num_mb, out_dir, mode, fake_nodes=False, extra_env=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0", TFK_DP_MIN_SHARD="64")
    if fake_nodes:  # a 1-GPU box: the ranks share the device and claim a host each (dataparallel._share_device)
        os.environ["TFK_FAKE_NODES"] = "1"
    os.environ.update(extra_env or {})
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from tfkaldi_amd.dataparallel import DataParallel, init_from_env
    _, _, local = init_from_env()
    assert dist.get_backend() == "nccl" and dist.get_world_size() == world
    dp = DataParallel(mode=mode)
    from tfkaldi_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util import make_pair
    from test_gpu_dp_two_ranks import KW
    eng, _ = make_pair(np.random.default_rng(3), torch_state=True, device=local, **KW)
    # one step by hand BEFORE Adam amplifies anything: after the collectives the reduce region must hold the serial run's
    # gradient sums -- the whole of an all-reduced span, this rank's 1/world of a reduce-scattered one
    from tfkaldi_amd.dataparallel import partition
    red = dp.reducer(eng)
    assert red.native and red.backend == "rccl"
    mbs = _data(num_mb, 100)
    start, end = partition(len(mbs), world)[rank]
    eng.set_later_microbatches(len(mbs) - end)
    for i, (X, y) in enumerate(mbs[start:end]):
        eng.accumulate(X, y, last=(i == end - start - 1))
    if start == end:  # more ranks than micro-batches: this rank contributes zeros
        red.idle(eng)
    red.finish_reduce()
    eng.synchronize()
    region = eng.reduce_view().cpu().numpy().copy()
    loss100 = red.finish_and_apply(eng)
    spans = np.array([[off, n, kind == "rs"] for (off, n), kind in zip(red.last_launched, red.last_span_kinds)])
    # what this rank owns of every reduce-scattered span: [span, offset, floats]
    shards = np.array([[i, o, m] for i, ((off, n), kind) in enumerate(zip(red.last_launched, red.last_span_kinds)) if kind == "rs"
                       for o, m in red.my_shards(off, n)] or np.zeros((0, 3)), dtype=np.int64)
    info = red.exchange_info()
    if os.environ.get("TFK_DP_ALGO") == "auto":  # timed at attach, the slowest rank's figures decide identically everywhere
        assert info["chosen_by"] == "tuned at attach" and len(info["tuned_us_slowest_rank"]) == 4, info
    else:
        assert info["reduce_scatter"] == os.environ.get("TFK_DP_ALGO", "rccl"), info
    assert info["wire"] == os.environ.get("TFK_DP_WIRE", "fp32")
    assert red.planes == (os.environ.get("TFK_DP_GATHER") == "planes" and mode == "sharded")
    losses = [dp.train_step(eng, _data(num_mb, step)) for step in range(3)]
    losses.append(dp.eval_step(eng, _data(num_mb, 9)))
    dp.gather_parameters(eng)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), region=region, spans=spans, shards=shards, loss100=np.array(loss100),
             **_collect(eng, losses))
    eng.close()
    dist.destroy_process_group()


OPTIONS = {"": {}, "direct": {"TFK_DP_ALGO": "direct"}, "direct+planes": {"TFK_DP_ALGO": "direct", "TFK_DP_GATHER": "planes"},
           "planes": {"TFK_DP_GATHER": "planes"}, "bf16wire": {"TFK_DP_WIRE": "bf16"}, "no-hold": {"TFK_DP_HOLD_LAST": "0"},
           "comm-stream-tail": {"TFK_DP_INLINE_TAIL": "0"}, "auto": {"TFK_DP_ALGO": "auto"},
           "bf16wire+planes": {"TFK_DP_WIRE": "bf16", "TFK_DP_GATHER": "planes"}}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world,num_mb,mode,options", [
    (2, 4, "sharded", ""), (2, 4, "allreduce", ""), (2, 2, "sharded", "direct"), (2, 4, "sharded", "direct+planes"),
    (2, 4, "sharded", "planes"), (2, 4, "sharded", "bf16wire"), (2, 4, "sharded", "no-hold"), (2, 4, "sharded", "comm-stream-tail"),
    (2, 1, "sharded", ""), (2, 4, "sharded", "auto"), (4, 4, "sharded", "bf16wire+planes"), (4, 4, "sharded", "direct"), (4, 6, "sharded", "planes"), (4, 8, "allreduce", ""),
    (8, 8, "sharded", "direct+planes"), (8, 11, "sharded", "")])
def test_real_rccl_ranks_match_serial(gpu, tmp_path, world, num_mb, mode, options):
    """`world` ranks over REAL RCCL: the data-parallel step == the serial step.  With enough GPUs one rank per device; on a
    1-GPU box the ranks share the device and each claims a host of its own (TFK_FAKE_NODES -> NCCL_HOSTID), so RCCL's
    duplicate-device check passes and the collectives travel through its socket transport on the loopback interface: RCCL's own
    bootstrap at world > 1, ncclReduceScatter / ncclAllGather / ncclAllReduce, the grouped ncclSend / ncclRecv of the direct
    algorithm and of the bf16 wire, plane gathers, the inline tail -- everything a 1-GPU box never ran before round 6."""
    import torch
    import torch.multiprocessing as mp
    fake = torch.cuda.device_count() < world
    mp.spawn(_rccl_worker, args=(world, _free_port(), num_mb, str(tmp_path), mode, fake, OPTIONS[options]), nprocs=world,
             join=True)
    eng = _engine(torch_state=True)
    mbs = _data(num_mb, 100)
    for i, (X, y) in enumerate(mbs):
        eng.accumulate(X, y, last=(i == len(mbs) - 1))
    eng.synchronize()
    region = eng.reduce_view().cpu().numpy().copy()
    num_params = eng.buckets()[-1][0]
    loss100 = eng.apply()
    want = []
    for step in range(3):
        mbs = _data(num_mb, step)
        for i, (X, y) in enumerate(mbs):
            eng.accumulate(X, y, last=(i == len(mbs) - 1))
        want.append(eng.apply())
    for X, y in _data(num_mb, 9):
        eng.eval_accumulate(X, y)
    want.append(eng.eval_finish())
    ref = _collect(eng, want)
    eng.close()
    lr = 1e-3
    bf16_wire = "bf16wire" in options
    # the summed gradients before the optimiser: same addends as the serial accumulation, another order (a block of
    # micro-batches per rank, then over the ranks) -- 1e-5 on the scale of the span, as the all-reduce variant of
    # tests/test_gpu_dp_two_ranks.py; bf16 payloads: 2^-8 of the other ranks' contributions (test_gpu_native_exchange.py)
    tol = 2.0 ** -7 if bf16_wire else 1e-5
    for rank in range(world):
        got = np.load(os.path.join(str(tmp_path), "rank%d.npz" % rank))
        assert abs(float(got["loss100"]) - loss100) <= 3e-6 * abs(loss100)
        kinds = [bool(k) for _, _, k in got["spans"]]
        assert any(kinds) == (mode == "sharded")
        checked = 0
        for i, (off, n, rs) in enumerate(got["spans"]):
            off, n = int(off), int(n)
            if off >= num_params:
                continue
            scale = np.abs(region[off:off + n]).max() + 1e-30
            parts = [slice(int(o), int(o + m)) for j, o, m in got["shards"] if j == i] if rs else [slice(off, off + n)]
            assert parts
            for part in parts:
                err = np.abs(got["region"][part] - region[part]).max()
                assert err <= tol * scale, (mode, rank, off, n, bool(rs), err, scale)
                if rs and "direct" in options and num_mb == world:
                    # one micro-batch per rank, the owner adds in rank order: the serial run's additions in its order
                    assert np.array_equal(got["region"][part], region[part]), (rank, off, n)
                checked += part.stop - part.start
        assert checked > 0
        assert np.allclose(got["losses"], ref["losses"], rtol=2e-3 if bf16_wire else 2e-6, atol=0), (got["losses"], ref["losses"])
        for k in ref:
            if k == "losses":
                continue
            if k.startswith("m"):  # (BN moving averages: of layers above the first, they see the updated weights below them)
                assert np.allclose(got[k], ref[k], rtol=1e-3 if bf16_wire else 1e-5, atol=1e-5 if bf16_wire else 1e-7), k
            else:
                err = np.abs(got[k] - ref[k])
                assert np.mean(err > 0.02 * lr * 3) < (0.05 if bf16_wire else 0.01) and err.max() <= 2 * lr * 3, k
    # every rank ends with the same parameters
    first = np.load(os.path.join(str(tmp_path), "rank0.npz"))
    for rank in range(1, world):
        got = np.load(os.path.join(str(tmp_path), "rank%d.npz" % rank))
        for k in ref:
            if k != "losses":
                assert np.array_equal(got[k], first[k]), (rank, k)


_NNET_SCRIPT = r"""
import configparser, os, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
from tfkaldi_amd import compat, synthetic
compat.install()
from neuralNetworks import nnet
from tfkaldi_amd.processing import batchdispenser, feature_reader, target_coder
out = sys.argv[1]
F_RAW, CONTEXT, O = 8, 2, 12
lengths = np.random.default_rng(0).integers(6, 30, size=26)
# (every rank writes its own copy of the same deterministic corpus: two ranks writing ONE directory race with each other's reads)
paths = synthetic.write_corpus(os.path.join(out, "data_rank" + os.environ.get("RANK", "0")), 26, O, feat_dim=F_RAW, lengths=lengths,
                               num_speakers=3)
conf = configparser.ConfigParser()
conf.add_section("directories"); conf.set("directories", "expdir", out)
conf.add_section("nnet")
for k, v in dict(name="dnn", context_width=str(CONTEXT), num_hidden_units="32", num_hidden_layers="2", add_layer_period="3",
                 starting_step="0", nonlin="relu", l2_norm="False", dropout="1", batch_norm="True", num_epochs="2",
                 initial_learning_rate="0.01", learning_rate_decay="1", batch_size="4", numutterances_per_minibatch="2",
                 valid_batches="1", valid_frequency="2", valid_adapt="False", valid_retries="3", check_freq="4",
                 visualise="False", seed="11").items():
    conf.set("nnet", k, v)
net = nnet.Nnet(conf, F_RAW, O)
reader = feature_reader.FeatureReader(paths["feats_scp"], paths["cmvn_scp"], paths["utt2spk"], CONTEXT, 30)
disp = batchdispenser.AlignmentBatchDispenser(reader, target_coder.AlignmentCoder(lambda x, y: x, O), 4, paths["alignments"])
net.train(disp)
"""


@pytest.mark.timeout(600)
def test_nnet_train_under_one_rccl_rank_with_plane_gathers(gpu, tmp_path):
    """`Nnet.train` itself -- layer-wise growth (control ops re-initialise the output layer), validation, check
    points (roll-back after a worse validation loss: tests/test_gpu_nnet_e2e.py) -- under the in-library exchange with ONE RCCL rank in the configuration that leaves the fp32 masters with their owner
    between steps (emulated fp32, TFK_DP_GATHER=planes, TFK_DP_ALGO=direct): every place that reads or writes parameters from
    outside the optimiser must bring them home first (trainer.gather_parameters), or the param_access_hook raises.  With one rank
    nothing is summed across ranks, so the final model equals the single-process run's bit for bit."""
    script = tmp_path / "run_nnet.py"
    script.write_text(_NNET_SCRIPT.format(root=ROOT))
    models = {}
    for tag, extra in (("plain", {}), ("dp", dict(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1",
                                                  LOCAL_RANK="0", TFK_FORCE_DP="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
                                                  TFK_DP_GATHER="planes", TFK_DP_ALGO="direct", TFK_DP_MIN_SHARD="64"))):
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TFK_FORCE_DP")}
        env.update(extra)
        out_dir = tmp_path / tag
        out_dir.mkdir()
        r = subprocess.run([sys.executable, str(script), str(out_dir)], env=env, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
        assert "adding layer" in r.stdout and "validation loss at step" in r.stdout
        models[tag] = (dict(np.load(str(out_dir / "dnn" / "final"))), [l for l in r.stdout.splitlines() if "loss" in l])
    plain, dp = models["plain"], models["dp"]
    assert plain[1] == dp[1], (plain[1][-3:], dp[1][-3:])  # every printed loss line, training and validation
    assert sorted(plain[0]) == sorted(dp[0])
    for k, v in plain[0].items():
        np.testing.assert_array_equal(dp[0][k], v, err_msg=k)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("options", ["", "direct+planes"])
def test_nnet_train_under_two_real_rccl_ranks(gpu, tmp_path, options):
    """`Nnet.train` -- packed feed (each rank reads its own utterances), layer-wise growth, validation, check points --
    as `torchrun --nproc-per-node 2` over REAL RCCL (two GPUs, or one GPU with TFK_FAKE_NODES): every step has two
    micro-batches, one per rank, so the exchanged sums are a + b against the serial run's a + b -- the training losses
    printed by rank 0 must agree with the single-process run's to fp32 round-off (the BN moving averages are composed from
    increments instead of updated one after the other, which moves the validation losses in their last digits)."""
    import re
    import torch
    script = tmp_path / "run_nnet.py"
    script.write_text(_NNET_SCRIPT.format(root=ROOT))
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TFK_FORCE_DP")}
    runs = {}
    for tag in ("plain", "dp"):
        env = dict(base)
        out_dir = tmp_path / tag
        out_dir.mkdir()
        cmd = [sys.executable, str(script), str(out_dir)]
        if tag == "dp":
            env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", TFK_DP_MIN_SHARD="64", TFK_DP_COMM="native-only", **OPTIONS[options])
            if torch.cuda.device_count() < 2:
                env["TFK_FAKE_NODES"] = "1"
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                   "127.0.0.1", "--master-port", str(_free_port())] + cmd[1:]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
        assert "adding layer" in r.stdout and "validation loss at step" in r.stdout
        lines = [l for l in r.stdout.splitlines() if "loss" in l]
        runs[tag] = (dict(np.load(str(out_dir / "dnn" / "final"))), lines)
    plain, dp = runs["plain"], runs["dp"]
    assert len(plain[1]) == len(dp[1]) and len(plain[1]) >= 8, (plain[1], dp[1])
    number = re.compile(r"[-+]?\d+\.\d+(?:[eE][-+]?\d+)?")
    for a, b in zip(plain[1], dp[1]):
        va, vb = [float(x) for x in number.findall(a)], [float(x) for x in number.findall(b)]
        assert number.sub("#", a) == number.sub("#", b), (a, b)  # same message, same step
        assert np.allclose(va, vb, rtol=2e-3, atol=1e-5), (a, b)
    assert sorted(plain[0]) == sorted(dp[0])
    for k, v in plain[0].items():
        assert dp[0][k].shape == v.shape, k
        if v.dtype.kind == "f" and v.size > 1:
            assert np.abs(dp[0][k] - v).mean() <= 2e-3 * (np.abs(v).mean() + 1e-3) + 1e-4, k


CTC_KW = dict(input_dim=20, num_layers=2, num_units=32, output_dim=9, nonlin="tanh", batch_norm=True,
              init_learning_rate=1e-3, num_steps=50)


def _ctc_data(num_mb, seed):
    """micro-batches of two utterances each for the CTC loss: (frames, utterance lengths, labels back to back, label counts)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(num_mb):
        utt, lab = [30 + 3 * i, 17 + i], [5 + i % 3, 3]
        X = (rng.standard_normal((sum(utt), CTC_KW["input_dim"])) * 1.5).astype(np.float32)
        labels = np.concatenate([rng.integers(0, CTC_KW["output_dim"] - 1, size=n) for n in lab]).astype(np.int32)
        out.append((X, utt, labels, lab))
    return out


def _ctc_worker(rank, world, port, num_mb, out_dir, mode, fake_nodes):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0", TFK_DP_MIN_SHARD="64", TFK_DP_COMM="native-only")
    if fake_nodes:
        os.environ["TFK_FAKE_NODES"] = "1"
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from tfkaldi_amd.dataparallel import CtcMicroBatch, DataParallel, init_from_env
    from util import make_pair
    _, _, local = init_from_env()
    dp = DataParallel(mode=mode)
    eng, _ = make_pair(np.random.default_rng(5), output_too=False, max_frames=256, torch_state=True, device=local, **CTC_KW)
    losses = [dp.train_step(eng, [CtcMicroBatch(*mb) for mb in _ctc_data(num_mb, step)]) for step in range(3)]
    assert dp.reducer(eng).native
    losses.append(dp.eval_step(eng, [CtcMicroBatch(*mb) for mb in _ctc_data(num_mb, 9)]))
    dp.gather_parameters(eng)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **_collect(eng, losses))
    eng.close()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,num_mb,mode", [(2, 4, "sharded"), (4, 5, "sharded"), (2, 3, "allreduce")])
def test_ctc_steps_over_real_rccl_ranks(gpu, tmp_path, world, num_mb, mode):
    """BASELINE configs[4] (the CTCTrainer path, 1 -> 8 GPUs): micro-batches under the CTC loss dealt to REAL RCCL ranks
    (uneven blocks, an idle-free 4-rank case) == the serial run: the loss is normalised by the label count SUMMED over the ranks
    (the `frames` scalar of the reduce region), the gradients are summed like the cross-entropy path's"""
    import torch
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util import make_pair
    mp.spawn(_ctc_worker, args=(world, _free_port(), num_mb, str(tmp_path), mode, torch.cuda.device_count() < world), nprocs=world,
             join=True)
    eng, _ = make_pair(np.random.default_rng(5), output_too=False, max_frames=256, **CTC_KW)
    want = []
    for step in range(3):
        mbs = _ctc_data(num_mb, step)
        for i, (X, utt, labels, lab) in enumerate(mbs):
            eng.accumulate_ctc(X, utt, labels, lab, last=(i == len(mbs) - 1))
        want.append(eng.apply())
    for X, utt, labels, lab in _ctc_data(num_mb, 9):
        eng.eval_accumulate_ctc(X, utt, labels, lab)
    want.append(eng.eval_finish())
    ref = _collect(eng, want)
    eng.close()
    lr = CTC_KW["init_learning_rate"]
    for rank in range(world):
        got = np.load(os.path.join(str(tmp_path), "rank%d.npz" % rank))
        assert np.allclose(got["losses"], ref["losses"], rtol=1e-5, atol=0), (got["losses"], ref["losses"])
        for k in ref:
            if k == "losses":
                continue
            if k.startswith("m"):
                assert np.allclose(got[k], ref[k], rtol=1e-5, atol=5e-7), k
            else:
                err = np.abs(got[k] - ref[k])
                assert np.mean(err > 0.02 * lr * 3) < 0.01 and err.max() <= 2 * lr * 3, k
