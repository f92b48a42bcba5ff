"""Ragged batches against the fixed-N calls they replace, on one GPU (a measurement tool; bench.py stays the headline).

B = 10 000 seeded synthetic triplets with n ~ U[100, 300] correspondences, per method:
  (a) ragged   one tff_pose_batch_ragged_dev call for the whole packed batch (n_max passed: no synchronisation);
  (b) grouped  the same triplets grouped by n, one fixed-N _dev call per distinct n (~200 calls);
  (c) fixed    a fixed-N batch of 10 000 x 200 (what the ragged call costs per triplet at the mean n).
Each figure is the median of --reps timed regions of --steps calls (HIP events around the region, after a warm-up), in triplets/s.
Methods: those the ragged entry point supports (api.RAGGED_METHODS).

  python tools/bench_ragged.py [--B 10000] [--steps 10] [--reps 7] [--methods LinearTFTPoseEstimation,...]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tft_vs_fund_amd import api  # noqa: E402
from tft_vs_fund_amd.scenes import generate_scene_batch  # noqa: E402


def timed(fn, steps, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--methods", default=",".join(api.RAGGED_METHODS))
    args = ap.parse_args()
    B = args.B
    rng = np.random.default_rng(2024)
    ns = rng.integers(100, 301, size=B)
    C, CalM, _, _ = generate_scene_batch(B, 300, noise=1.0, seed=5)
    items = [C[b, :ns[b]] for b in range(B)]
    corresp, offsets = api.pack_ragged(items)
    n_max = int(ns.max())
    dev = torch.device("cuda", 0)
    d_corr = torch.from_numpy(corresp).to(dev)
    d_off = torch.from_numpy(offsets).to(dev)
    d_calm = torch.from_numpy(CalM).to(dev)
    groups = []
    for n in np.unique(ns):
        idx = np.nonzero(ns == n)[0]
        groups.append(torch.from_numpy(np.ascontiguousarray(C[idx, :n])).to(dev))
    fixed = torch.from_numpy(np.ascontiguousarray(C[:, :200])).to(dev)
    ctx = api.Context(0)
    results = {"B": B, "n": "U[100, 300]", "distinct_n": len(groups), "mean_n": float(ns.mean()), "steps": args.steps, "reps": args.reps,
               "unit": "triplets/s", "methods": {}}
    for method in args.methods.split(","):
        r = {}
        ms, all_ms = timed(lambda: ctx.pose_batch_ragged(method, d_corr, d_off, d_calm, reconst=False, n_max=n_max), args.steps, args.reps)
        r["ragged"] = {"ms": ms, "per_s": B / ms * 1e3, "reps_ms": all_ms}

        def grouped():
            for g in groups:
                ctx.pose_batch(method, g, d_calm, reconst=False)
        ms, all_ms = timed(grouped, max(1, args.steps // 5), args.reps, warmup=1)
        r["grouped"] = {"ms": ms, "per_s": B / ms * 1e3, "calls": len(groups), "reps_ms": all_ms}
        ms, all_ms = timed(lambda: ctx.pose_batch(method, fixed, d_calm, reconst=False), args.steps, args.reps)
        r["fixed_200"] = {"ms": ms, "per_s": B / ms * 1e3, "reps_ms": all_ms}
        r["ragged_over_fixed"] = r["ragged"]["per_s"] / r["fixed_200"]["per_s"]
        r["ragged_over_grouped"] = r["ragged"]["per_s"] / r["grouped"]["per_s"]
        results["methods"][method] = r
    print(json.dumps(results))


if __name__ == "__main__":
    main()
