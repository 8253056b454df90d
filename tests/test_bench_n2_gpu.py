"""The N > 1 code path of bench.py -- the one the driver's 2/4/8-GPU scaling run executes -- run for real with two and four ranks.

A test run has ONE MI355X, so the ranks share it (RGBNM_BENCH_SAME_DEVICE=1) and talk over gloo
(RGBNM_BENCH_BACKEND=gloo); on the 8-GPU node the same code runs one rank per GPU over RCCL.  No scaling number is
asked of this test: the point is that process-group set-up, the FlatGradSync self-check, the HIP-graph capture with the
exchange after the replay, the schedule calibration (four candidates), the max-over-ranks timing and the JSON line all
execute.  Reference loop: train.py:137 (DDP wrap), :145-176 (step)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, timeout=900, nproc=2, **more_env):
    env = dict(os.environ, RGBNM_BENCH_SAME_DEVICE="1", RGBNM_BENCH_BACKEND="gloo",
               HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    env.update(more_env)
    # --standalone: the launcher binds a free port itself (no probe-then-bind race)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nnodes=1", "--nproc-per-node", str(nproc),
           os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "4", "--warmup", "1",
           "--prewarm-sec", "0.2", "--no-cpu-baseline"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (r.stdout[-2000:], r.stderr[-2000:])       # rank 0 prints ONE line
    return json.loads(lines[0])


def test_bench_two_ranks_flat_exchange_with_calibration():
    d = _run([])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "weak"
    cfg = d["config"]
    assert cfg["global_batch"] == 2 * cfg["per_gpu_batch"] == 512 and cfg["parallelism"] == "dp2"
    assert cfg["grad_sync"].startswith("flat"), cfg["grad_sync"]        # the self-check passed: no fallback to torch DDP
    cal = cfg["grad_sync_calibration_ms_per_step"]
    # incl. "HIP graph replay, then one all-reduce" and the two "all-reduce under the next step's data stage" schedules
    assert len(cal) == 6 and all(v > 0 for v in cal.values()), cal
    assert sum("next step's data stage" in k for k in cal) == 2, cal
    assert cfg["grad_sync"].split(": ", 1)[1] in cal
    assert d["parity_check"]["ok"] is True
    assert d["value"] > 0 and abs(d["value"] - 512 / (d["ms_per_step"] / 1e3)) < 0.01 * d["value"]
    loss = cfg["loss"]
    assert loss == loss and 0 < loss < 20


def test_bench_two_ranks_exchange_under_the_next_data_stage():
    """The schedule of VERDICT r4 item 4 (ii), pinned: HIP-graph replay of forward + backward, ONE all-reduce issued behind it and
    waited for only in front of the optimizer step, which is queued behind the NEXT step's data stage
    (parallel.DeferredFlatExchange; bit equality with the blocking schedule: tests/test_deferred_exchange_gloo_cpu.py)."""
    d = _run([], RGBNM_BENCH_SCHEDULE="HIP graph replay, all-reduce under the next step's data stage")
    cfg = d["config"]
    assert "all-reduce under the next step's data stage" in cfg["grad_sync"] and cfg["grad_sync"].startswith("flat"), cfg["grad_sync"]
    assert cfg["launch"].startswith("HIP graph replay"), cfg["launch"]
    assert d["parity_check"]["ok"] is True
    loss = cfg["loss"]
    assert loss == loss and 0 < loss < 20


def test_bench_two_ranks_torch_ddp_path():
    d = _run(["--grad-sync", "ddp", "--no-parity-check", "--no-trace"])
    assert d["n_gpus"] == 2 and d["config"]["grad_sync"] == "ddp"
    assert d["config"]["launch"] == "eager"
    loss = d["config"]["loss"]
    assert loss == loss and 0 < loss < 20


def test_bench_two_ranks_swinv2_gathered_flat_exchange():
    """bench.py --arch swinv2t at N = 2: the gathered flat exchange (parallel.GatheredFlatGradSync) passes its self-check against one
    blocking all-reduce and carries the step (config 5 no longer goes through torch DDP's bucket copies)."""
    d = _run(["--arch", "swinv2t", "--batch", "32", "--no-parity-check"])
    assert d["n_gpus"] == 2 and d["config"]["grad_sync"].startswith("flat-gathered"), d["config"]["grad_sync"]
    assert d["config"]["global_batch"] == 64
    loss = d["config"]["loss"]
    assert loss == loss and 0 < loss < 20


def test_bench_four_ranks_on_one_gpu():
    """The N > 2 code path on the one MI355X of a test run (gloo).  BASELINE config 3 names 8 ranks, but at most six processes may
    hold the GPU at once, this test's own included, so four ranks run it (per-rank batch 64, global batch 256 as in config 3):
    process group of 4, the per-rank shards (seed + rank), the flat-exchange self-check against one blocking all-reduce on every
    rank, the six-schedule calibration with its MIN / MAX reductions over the ranks, max-over-ranks timing and the one JSON line.
    Reference: train.py:137, :145-176, datasets.py:533-535."""
    d = _run(["--batch", "64", "--no-parity-check", "--no-trace"], timeout=1500, nproc=4, OMP_NUM_THREADS="1")
    assert d["n_gpus"] == 4 and d["steps"] == 4 and d["scaling"] == "weak"
    cfg = d["config"]
    assert cfg["global_batch"] == 4 * cfg["per_gpu_batch"] == 256 and cfg["parallelism"] == "dp4"
    assert cfg["grad_sync"].startswith("flat"), cfg["grad_sync"]
    cal = cfg["grad_sync_calibration_ms_per_step"]
    assert len(cal) == 6 and all(v > 0 for v in cal.values()), cal
    assert d["value"] > 0 and abs(d["value"] - 256 / (d["ms_per_step"] / 1e3)) < 0.01 * d["value"]
    loss = cfg["loss"]
    assert loss == loss and 0 < loss < 20
