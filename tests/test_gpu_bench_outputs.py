"""bench.py's plain run (headline only) and --dump-outputs: the line carries the headline keys and nothing that --full adds, the dumped
arrays are float32 and finite, and two runs with the same arguments dump the same outputs -- also after enough timed steps for the runs'
own trajectories to have drifted apart (float-atomic order + Adam), since the dump replays the last timed step from the seeded start."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = {"roofline", "steady_state", "trained_state", "bf16_transports", "psnr_30k", "reference_standin", "config3", "config4", "cpu_baseline"}


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT)
    runs = []
    for i in range(2):
        d = tmp_path / f"out{i}"
        out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "40", "--warmup", "2", "--images", "38", "--dump-outputs", str(d)],
                             env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 40 and line["warmup"] == 2 and line["n_gpus"] == 1
        assert line["unit"] == "rays/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
        assert line["ms_per_step"] > 0 and abs(line["value"] - 4096 * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
        assert not FULL_ONLY & set(line), FULL_ONLY & set(line)
        files = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert {"rgb", "params_sample", "loss_rgb_loss", "loss_interlevel_loss", "loss_distortion_loss"} <= set(files)
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
        assert files["rgb"].shape == (4096, 3) and files["params_sample"].size > 1_000_000
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        runs.append(files)
    a, b = runs
    assert set(a) == set(b)
    # same seeds -> same batch, same start: what is left is the last-bit order of the float-atomic gradient sums of one step
    np.testing.assert_allclose(a["rgb"], b["rgb"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(a["params_sample"], b["params_sample"], rtol=0, atol=1e-6)
    for k in a:
        if k.startswith("loss_"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=0, err_msg=k)
