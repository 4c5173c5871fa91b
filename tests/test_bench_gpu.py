"""GPU: a plain bench.py run end to end (the smallest config, C2 at 8 samples): the result line
carries the headline keys and none of the --full figures, --steps sets the number of timed
steps, and --dump-outputs writes the last timed step's outputs as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(dev, tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--config", "c2", "--batch", "8", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["metric"].startswith("multimodal samples/sec") and res["unit"] == "samples/s"
    assert res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region (both rounded in the line)
    assert res["value"] == pytest.approx(8 / (res["ms_per_step"] * 1e-3), rel=1e-3)
    assert "roofline" not in res and "cpu_baseline" not in res
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == ["grad_norm", "grads_sample", "logits", "loss", "params_sample"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert got["logits"].shape == (8, 13)
    assert got["loss"][0] == pytest.approx(res["loss"], abs=1e-5)
    assert got["params_sample"].shape == got["grads_sample"].shape
    assert got["grads_sample"].any() and got["grad_norm"][0] > 0
