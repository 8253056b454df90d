"""bench.py --dump-outputs: what the last timed step computed (loss, logits, parameters after the optimizer step, gradients), written as
float32 .npy files that two runs with the same arguments write alike.  The prewarm loop runs for a time, not a number of steps; bench.py
puts the model, the optimizer and the random streams back after it, so runs with different prewarm times must write the same bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PARAMS_VITTI = 5642728          # JPEG-Ti: under bench.py's DUMP_ELEMS cap, written whole


def _bench(out, prewarm_sec):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--prewarm-sec", str(prewarm_sec), "--no-cpu-baseline", "--no-parity-check", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(lines[0])


def test_dump_outputs_are_the_same_bits_whatever_the_prewarm(tmp_path):
    a = _bench(tmp_path / "a", 0)
    b = _bench(tmp_path / "b", 1.0)
    assert a["steps"] == b["steps"] == 3 and a["ms_per_step"] > 0 and b["ms_per_step"] > 0
    names = ["grads", "logits", "loss", "params"]
    assert sorted(f[:-len(".npy")] for f in os.listdir(tmp_path / "a")) == names
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), (n, float(np.abs(x - y).max()))
        total += os.path.getsize(tmp_path / "a" / f"{n}.npy")
    assert total <= 64e6
    assert np.load(tmp_path / "a" / "logits.npy").shape == (256, 1000)
    assert np.load(tmp_path / "a" / "params.npy").shape == np.load(tmp_path / "a" / "grads.npy").shape == (N_PARAMS_VITTI,)
    assert abs(float(np.load(tmp_path / "a" / "loss.npy")) - a["config"]["loss"]) < 1e-4
