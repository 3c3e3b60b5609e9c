"""bench.py end to end on a small workload: the one-GPU line carries the contract's fields, and the N > 1 control flow (eager leg,
guarded graph leg, one JSON line from rank 0) runs with two ranks sharing the box's one GPU over gloo (RNAD_BENCH_REHEARSAL)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
SMALL = ["--depth", "4", "--batch-log2", "14", "--steps", "40", "--warmup", "3", "--other-steps", "4", "--cpu-lanes-log2", "9"]
FULL = SMALL + ["--full"]  # (roofline, cpu_baseline, the N > 1 base leg: what a plain run leaves out)


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line expected:\n{out[-3000:]}"
    return json.loads(lines[0])


@pytest.mark.timeout(900)
def test_one_gpu_line_has_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *FULL], capture_output=True, text=True, timeout=850)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _json_line(r.stdout)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline"):
        assert key in j, key
    assert j["n_gpus"] == 1 and j["steps"] == 40 and j["warmup"] == 3 and j["value"] > 0 and j["unit"] == "env-steps/s"
    assert j["net_evaluation"]["step_replayed_from_hipGraph"] is True
    roof = j["roofline"]
    assert roof["bound"] in ("hbm", "mfma", "valu", "l1/latency") and roof["unit"] in ("GB/s", "TFLOP/s", "Gwave-inst/s") and 0 < roof["frac"] < 1
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9
    cpu = j["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["sample"]
    assert abs(j["value"] - j["config"]["global_batch"] * j["config"]["T"] * j["steps"] / (j["ms_per_step"] * 1e-3 * j["steps"])) < 1e-6 * j["value"]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("scaling", ("weak", "strong"))
def test_two_rank_control_flow(scaling):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, RNAD_BENCH_REHEARSAL="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scaling", scaling, *FULL]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=850, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 2 and j["scaling"] == scaling and j["config"]["global_batch"] == 2 * j["config"]["per_gpu_batch"]
    assert j["config"]["global_batch"] == ((2 << 14) if scaling == "weak" else (1 << 14))
    assert j["value"] > 0 and "eager" in j["legs_ms_per_step"] and "cpu_baseline" not in j
    assert j["collectives"]["ranks"] == 2 and j["collectives"]["backend"] == "gloo" and j["collectives"]["rccl_ranks"] is None
    if scaling == "strong":  # rank 0 also timed the same global batch alone: the N = 1 point of the curve
        base = j["strong_scaling"]["base"]
        assert base["global_batch"] == 1 << 14 and base["ms_per_step"] > 0 and j["strong_scaling"]["speedup_vs_one_gpu_same_batch"] > 0
    else:
        assert "strong_scaling" not in j
    assert abs(j["value"] - j["config"]["global_batch"] * j["config"]["T"] / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]


@pytest.mark.timeout(1500)
def test_eight_ranks_with_no_other_flags_run_configs_2():
    """`bench.py --gpus 8` as the driver launches it: BASELINE.json configs[2] -- one 2^22 batch, 2^19 lanes per rank, strong scaling --
    rehearsed with the eight ranks sharing this box's GPU over gloo.  Rank 0's stand-alone leg is the 2^22 batch on ONE GPU in the
    default mode (the N = 1 point of that curve)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, RNAD_BENCH_REHEARSAL="1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "20", "--warmup", "2", "--other-steps", "2", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1400, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    j = _json_line(r.stdout)
    cfg = j["config"]
    assert j["n_gpus"] == 8 and j["scaling"] == "strong" and "configs[2]" in cfg["workload"]
    assert cfg["global_batch"] == 1 << 22 and cfg["per_gpu_batch"] == 1 << 19 and cfg["T"] == 12
    assert j["net_evaluation"]["in_effect"] == "True" and j["collectives"]["ranks"] == 8
    base = j["strong_scaling"]["base"]
    assert base["global_batch"] == 1 << 22 and base["net_mode_in_effect"] == "True" and base["step_replayed_from_hipGraph"] is True
    assert base["ms_per_step"] > 0 and j["value"] > 0
    assert abs(j["value"] - cfg["global_batch"] * cfg["T"] / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]


@pytest.mark.timeout(1500)
def test_eight_ranks_with_row_sharding():
    """The same rehearsal with `--shard-rows`: every rank evaluates 1/8 of the 2S rows, all-gathers the record tables and all-reduces the
    per-row sums (gloo here; the RCCL path differs only in the in-place all_gather_into_tensor)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, RNAD_BENCH_REHEARSAL="1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "10", "--warmup", "2", "--other-steps", "2",
           "--shard-rows", "--no-base-leg", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1400, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 8 and j["collectives"]["shard_rows"] is True and "all_gather" in j["collectives"]["per_step"]
    assert j["net_evaluation"]["in_effect"] == "True" and j["value"] > 0


def _dumped(path):
    import numpy as np

    out = {}
    for f in sorted(os.listdir(path)):
        assert f.endswith(".npy"), f
        out[f[:-4]] = np.load(os.path.join(path, f))
    return out


@pytest.mark.timeout(900)
def test_plain_line_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    """Without --full the line carries the headline alone (no roofline, kernel table, side legs or CPU baseline), --steps is the number of
    timed steps, and --dump-outputs writes what the last timed step computed: the same arrays, bit for bit, in two runs with the same
    arguments."""
    import numpy as np

    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SMALL, "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=400)
        assert r.returncode == 0, r.stderr[-3000:]
        j = _json_line(r.stdout)
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in j, key
        for key in ("roofline", "kernels", "cpu_baseline", "other_modes", "k1_observe", "host_enqueue_ms_per_step", "other_configs"):
            assert key not in j, key
        assert j["steps"] == 40 and j["warmup"] == 3 and j["unit"] == "env-steps/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
        assert j["net_evaluation"]["step_replayed_from_hipGraph"] is True
        assert abs(j["value"] - j["config"]["global_batch"] * j["config"]["T"] / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
        dumps.append(_dumped(d))
    a, b = dumps
    assert sorted(a) == sorted(b)
    assert {"lanes", "indices", "action_idx", "rewards", "policy"} <= set(a)
    assert any(k.startswith("net.") for k in a) and any(k.startswith("net_target.") for k in a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{k} differs between two runs with the same arguments"
    T, n = a["indices"].shape
    assert n == a["lanes"].size == 1 << 14 and a["policy"].shape == (T, n, 3) and a["rewards"].shape == (T, n)
    live = a["indices"] != 0
    assert live[0].all() and np.isfinite(a["policy"]).all()
    np.testing.assert_allclose(a["policy"].sum(-1)[live], 1.0, atol=1e-5)


@pytest.mark.timeout(900)
def test_two_rank_plain_line_dumps_rank_0_outputs(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, RNAD_BENCH_REHEARSAL="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", *SMALL, "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=850, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["steps"] == 40 and "eager" in j["legs_ms_per_step"]
    assert "strong_scaling" not in j and "cpu_baseline" not in j and j["collectives"]["allreduce_us"] is None
    d = _dumped(tmp_path)
    assert d["indices"].shape[1] == d["lanes"].size == j["config"]["per_gpu_batch"]
