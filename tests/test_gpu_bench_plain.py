"""A plain `bench.py --gpus 1 --steps K --warmup W` run: only the headline measurement (no roofline,
drop-in leg, CPU baseline or extra timed regions: those need --full), and `--dump-outputs DIR` writes
the records the last timed frame left, which are exactly what the same frame rendered here gives."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, STEPS, WARMUP = 72, 40, 8, 2, 1  # not multiples of the 8x8 block; two streams (short frames)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_frame(tmp_path):
    import torch
    import bench
    from vanrijn_amd import records as R
    from vanrijn_amd import scenes
    from vanrijn_amd.render import Tile, render_tile_device

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1", "--width", str(W),
           "--height", str(H), "--spp", str(SPP), "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "Msamples/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f64" and out["steps"] == STEPS and out["warmup"] == WARMUP and out["n_gpus"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - W * H * SPP / (out["ms_per_step"] * 1e3)) < 1e-3 * out["value"] + 1e-3
    for k in ("roofline", "drop_in", "cpu_baseline", "sequential", "weak_scaling", "traced_msamples_per_s"):
        assert k not in out, k
    assert "other_build_seconds" not in out["scene_build"]

    sums = np.load(tmp_path / "record_sums.npy")
    mean = np.load(tmp_path / "mean_colour.npy")
    assert sorted(os.listdir(tmp_path)) == ["mean_colour.npy", "record_sums.npy"]
    assert sums.dtype == np.float64 and sums.shape == (W * H, 4)
    assert mean.dtype == np.float64 and mean.shape == (W * H, 3)
    # the last timed frame is step 1 + WARMUP + STEPS - 1: its sample indices on the one rank
    step = WARMUP + STEPS
    state = torch.zeros(H * W * 8, dtype=torch.float64, device="cuda:0")
    ds = scenes.bench_scene().device_scene(0, device_sah=True)
    render_tile_device(ds, Tile(0, W, 0, H), H, W, SPP, bench.SEED, step * SPP, state.data_ptr(),
                       torch.cuda.current_stream().cuda_stream, device=0)
    torch.cuda.synchronize()
    ref = R.sums(state).cpu().numpy()
    assert np.array_equal(ref[:, 3], np.full(W * H, float(SPP)))
    assert np.array_equal(sums, ref)
    assert np.array_equal(mean, ref[:, 0:3] * (1.0 / ref[:, 3:4]))
