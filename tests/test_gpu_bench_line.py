"""The BENCH line closes on itself (round-4 verdict, weak #3): run bench.py as the driver does (one GPU, default streams) with a short timed region
and check the relations a reader should be able to verify from the line alone -- value x ms_per_step = the batch, the roofline from a launch that
has the GPU to itself (kernel_ms x steps / in_flight <= ms_per_step x steps, frac = achieved / peak, achieved = algorithmic bytes / kernel_ms),
the overlap factor, the repetitions with the median reported."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_bench_line_is_self_consistent():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "10", "--warmup", "2", "--reps", "5", "--no-secondary", "--no-cpu-baseline",
                        "--full"],
                       capture_output=True, text=True, timeout=560, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    B, K, S = d["config"]["batch_per_gpu"], d["steps"], d["in_flight"]
    assert d["n_gpus"] == 1 and K == 10 and S == 2 and d["config"]["failed_triplets"] == 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - B) < 1e-6 * B
    rep = d["repetitions"]
    assert rep["n"] == 5 and rep["reported"] == "median" and abs(np.median(rep["ms_per_step_each"]) - d["ms_per_step"]) < 1e-12
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert abs(rf["achieved"] - rf["algorithmic_bytes_per_launch"] / (rf["kernel_ms"] * 1e-3) / 1e9) < 1e-6 * rf["achieved"]
    assert rf["algorithmic_bytes_per_launch"] == B * (48 * d["config"]["correspondences"] + 216 + 216 + 192)
    # one launch alone is longer than a step of the overlapped region, but not by more than the batches in flight
    assert rf["kernel_ms"] * K / S <= d["ms_per_step"] * K * 1.02
    assert abs(d["overlap_factor"] - rf["kernel_ms"] / d["ms_per_step"]) < 1e-9 and 1.0 <= d["overlap_factor"] <= S
    # the one-batch-at-a-time figure is reported beside it and is the slower one
    assert d["single_stream"]["ms_per_batch"] >= d["ms_per_step"] and d["single_stream"]["ms_per_batch"] <= rf["kernel_ms"] * 1.05


@pytest.mark.timeout(600)
def test_plain_bench_run_dumps_what_pose_batch_returns(tmp_path):
    """A plain run (no --full) times --steps steps once and prints the headline keys; --dump-outputs writes the last timed step's
    outputs, which equal api.Context.pose_batch on the same seeded batch (bench.py's rank 0 draws it with seed 1000)."""
    import torch
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.scenes import generate_scene_batch
    B, N, K = 1000, 60, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(K), "--warmup", "1", "--batch", str(B), "--ncorr", str(N),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=560, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == K and d["repetitions"]["n"] == 1 and d["config"]["failed_triplets"] == 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - B) < 1e-6 * B and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert not {"roofline", "single_stream", "secondary", "cpu_baseline"} & set(d)
    C, CalM, _, _ = generate_scene_batch(B, N, noise=1.0, seed=1000)
    out = api.Context(0).pose_batch("LinearTFTPoseEstimation", torch.from_numpy(C).cuda(), torch.from_numpy(CalM).cuda(), reconst=False)
    torch.cuda.synchronize()
    for name, shape in (("R_t_2", (B, 3, 4)), ("R_t_3", (B, 3, 4)), ("T", (B, 3, 3, 3)), ("status", (B,))):
        got = np.load(os.path.join(str(tmp_path), name + ".npy"))
        want = out[name].cpu().numpy().astype(np.float64)
        assert got.dtype == np.float64 and got.shape == shape
        assert np.abs(got - want).max() <= 1e-12, name
