"""GPU: a plain `bench.py` run end to end at config 3's size (few steps): the result line and the --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)      # (a fresh process: its own HIP context)
    assert p.returncode == 0, p.stdout[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert (d["steps"], d["warmup"], d["n_gpus"], d["higher_is_better"], d["unit"]) == (3, 2, 1, True, "examples/sec")
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(65536 * 1e3 / d["ms_per_step"], rel=1e-9)
    assert d["state"]["rows_with_optimizer_state"] >= 0.99                  # the headline is the steady state
    assert not {"cold_start", "kernel_ms_per_step", "roofline", "configs", "cpu_baseline", "other_distribution"} & set(d)
    loss, logits = np.load(tmp_path / "loss.npy"), np.load(tmp_path / "logits.npy")
    assert loss.dtype == logits.dtype == np.float32 and loss.shape == (1,) and logits.shape == (65536,)
    assert float(loss[0]) == d["final_loss"] and np.isfinite(logits).all() and logits.std() > 0
