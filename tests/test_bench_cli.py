"""bench.py's two kinds of run: a plain run (set up, warm up, time the steps, --dump-outputs, the line) and `--full` (every other leg)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

# what a plain run leaves out of its line (null), each filled by --full
FULL_ONLY = ("roofline", "cpu_baseline", "parity", "pixel_parity", "cross_attention_block", "elide_dead_forwards_timing",
             "executed_flops_per_step", "whole_step_tflops_per_gpu", "whole_step_mfma_frac")
EXTRAS = ("intra_image_split_estimate", "graph_replay", "batched_2_requests", "plain_pass", "end_to_end", "end_to_end_one_pass_guidance")


def _bench(args, tmp_path, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout, cwd=str(tmp_path))


def _line(r):
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    return lines[0]


@pytest.mark.parametrize("extra", [["--config", "1"], ["--config", "2"], ["--config", "5"], ["--elide"], ["--roofline-only"]])
def test_other_measurements_need_full(extra, tmp_path):
    """Other configurations, elided timing and the roofline-only run are --full measurements: without it the command says so and
    exits before it touches a GPU."""
    r = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1"] + extra, tmp_path, timeout=300)
    assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-2000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_nothing_else(tmp_path):
    """A plain run prints the headline line with every --full figure null and no secondary legs; --dump-outputs still writes the
    latents of the last timed step."""
    import numpy as np
    out = tmp_path / "dump"
    d = _line(_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)], tmp_path, timeout=900))
    assert d["full"] is False and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["metric"] == "denoising steps/sec (SDXL 1024^2, 50-step, 4 regions)" and d["unit"] == "steps/s"
    assert d["higher_is_better"] is True and d["dtype"] == "bf16" and d["finite"] is True
    assert d["value"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["timed_schedule_indices"] == [0, 25]
    for k in FULL_ONLY:
        assert d[k] is None, k
    assert not set(EXTRAS) & set(d)
    lat = np.load(out / "latents.npy")
    assert lat.shape == (1, 4, 128, 128) and lat.dtype == np.float32 and np.isfinite(lat).all()


@pytest.mark.gpu
def test_full_run_keeps_its_legs(tmp_path):
    """--full still runs the roofline profile, the elided timing and cross_attention_block (the CPU baseline, the pixel parity and
    the secondary legs are trimmed here by their own switches: they take minutes)."""
    d = _line(_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-extras"], tmp_path, timeout=900))
    assert d["full"] is True and d["finite"] is True and d["value"] > 0
    assert d["roofline"]["achieved"] > 0 and d["roofline"]["per_kernel"]
    assert d["executed_flops_per_step"]["timed_steps"] == 2 and d["whole_step_tflops_per_gpu"] > 0
    assert d["elide_dead_forwards_timing"]["ms_per_step"] > 0
    assert d["cross_attention_block"]["A_4096x640"]["ms"] > 0 and d["cross_attention_block"]["B_1024x1280"]["ms"] > 0
    assert d["cpu_baseline"] is None and d["pixel_parity"] is None
