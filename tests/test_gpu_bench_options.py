"""GPU: bench.py's plain run (one process, a small env count): the headline line without the
--full measurements, and --dump-outputs (the state the last timed step left, as .npy)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, STEPS = 4096, 3


def test_plain_run_prints_the_headline_and_dumps_its_outputs(tmp_path):
    d = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "2",
           "--envs", str(E), "--dump-outputs", str(d)]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "env_steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == STEPS and out["full"] is False and out["ms_per_step"] > 0
    # value = the env-steps of the timed steps over their time
    assert abs(out["value"] - E * 20 * STEPS / (out["ms_per_step"] * STEPS / 1e3)) / out["value"] < 0.01
    # nothing that takes runs of its own
    assert not {"kernels", "phases", "roofline", "cpu_baseline"} & set(out)
    files = sorted(os.listdir(d))
    assert "sampler.obs.npy" in files and "store.cursor.npy" in files and any(f.startswith("net.") for f in files)
    total = 0
    arrs = {}
    for f in files:
        assert f.endswith(".npy")
        arrs[f[:-4]] = x = np.load(d / f)
        assert x.dtype in (np.float32, np.float64), (f, x.dtype)
        assert np.isfinite(x).all(), f
        total += x.nbytes
    assert total <= 64 * 1024 * 1024
    assert arrs["sampler.obs"].shape[0] == E
    ptr, size, won = (int(v) for v in arrs["store.cursor"][:3])
    assert size >= 5000 and won >= size  # the warm-up fill and the steps' windows
    rows = min(size, 4096)
    assert arrs["store.obs"].shape[:2] == (rows, 20) and arrs["store.rew"].shape == (rows, 20)
    assert np.abs(arrs["store.obs"]).max() > 0  # written windows, not untouched rows
    assert sorted(os.listdir(tmp_path)) == ["dump"]  # the run leaves nothing else in its working directory
