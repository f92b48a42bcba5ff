#!/usr/bin/env python3
"""
What quality-guided (PROSAC) sampling buys the robust estimators at a small budget, and what it costs: Context.robust_pose_scenes with and without
order= at n_hyp = 64, 256 and 1 000, LinearTFT and LinearF hypotheses at 4 px, 16 candidates, two refit rounds, over

  fountain, herzjesu   the triplet lists of tests/golden/epfl_all.npz (150 and 56 triplets, all their matches);
  synth50, synth65     `--scenes` scenes after the recipe of tools/config4_ransac.py: 400 matches, 0.5 px noise, 50 / 65 % of them displaced by
                       U(20, 80) px in views 2 and 3.

THE QUALITY IS SYNTHETIC.  The fixtures carry no match scores, so one is made from the ground truth: r = the largest of a match's six reprojection
residuals after triangulating it with the ground-truth cameras, quality = -log1p(r) + N(0, sigma) with sigma = 0.5 ("informative") and 1.5 ("weak");
log1p(r) is about 0.4 for a half-pixel inlier and about 4 for a 50 px outlier.  A real front end's score is something else; the table says what a
ranking of that strength does, not what a descriptor distance does.

One JSON line per (dataset, n_hyp, method, sampler): scenes with a pose (status 0), scenes with a GOOD pose (rotation error below 1 degree and
translation error below 5 degrees against the ground truth; per scene the mean over views 2 and 3, metrics.py), the median errors over the scenes with a
pose, ms per call (the median of `--reps` calls, the samplers alternated in one process after a warm-up call of each, host clock around a synchronise)
and, for the guided calls, the overhead against the uniform call at the same n_hyp.  The ranking is built once, outside the timed call.

Each (dataset, n_hyp) step is a child process under its own time limit; the first step that fails ends the run.

--sampler-only measures the sampler by itself instead (one child process): Context.sample_indices_guided -- the scene's pool table, the search and the
gather through the ranking, two launches -- against Context.sample_indices, one launch, for one scene of 400 and of 1 400 matches and 1 000 to 150 000
rows; one JSON line per shape with the device time between two events around the call (its torch.empty included), median [min, max] of 30 after a
warm-up, in microseconds.

  python tools/bench_robust_guided.py [--datasets fountain herzjesu synth50 synth65] [--hyp 64 256 1000] [--growth 200000] [--reps 7]
  python tools/bench_robust_guided.py --sampler-only
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

METHODS = ("LinearTFTPoseEstimation", "LinearFPoseEstimation")
SIGMAS = (("guided_informative", 0.5), ("guided_weak", 1.5))
THR = 4.0
GOOD = (1.0, 5.0)                # degrees: rotation, translation


def _cameras(CalM, R2, R3):
    return np.stack([CalM[0:3] @ np.eye(3, 4), CalM[3:6] @ R2, CalM[6:9] @ R3])


def load(name, args):
    """-> list of dict(scene (n, 6), CalM (9, 3), R_t0 [2 x (3, 4)])"""
    if name in ("fountain", "herzjesu"):
        from tft_vs_fund_amd.experiments import load_epfl_all
        return [dict(scene=np.ascontiguousarray(t["Corresp"].T), CalM=t["CalM"], R_t0=t["R_t0"])
                for t in load_epfl_all(os.path.join(ROOT, "tests", "golden", "epfl_all.npz"), name)]
    from tft_vs_fund_amd.scenes import generate_scene_batch
    share = {"synth50": 0.50, "synth65": 0.65}[name]
    items = []
    for k in range(args.scenes):
        C, CalM, Rt0, _ = generate_scene_batch(1, args.matches, noise=0.5, seed=7 + k)
        scene = C[0].copy()
        rng = np.random.default_rng(1 + k)
        bad = rng.choice(args.matches, int(share * args.matches), replace=False)
        scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
        items.append(dict(scene=np.ascontiguousarray(scene), CalM=np.ascontiguousarray(CalM), R_t0=Rt0))
    return items


def residuals(ctx, item):
    """the largest of each match's six reprojection residuals under the ground-truth cameras (experiments.epfl_inliers)"""
    P0 = _cameras(item["CalM"], item["R_t0"][0], item["R_t0"][1])
    X = ctx.triangulate(P0, item["scene"][None])
    X = (X.cpu().numpy() if hasattr(X, "cpu") else np.asarray(X))[0]
    Xh = np.vstack([X[0:3] / X[3:4], np.ones(X.shape[1])])
    proj = np.concatenate([(P @ Xh)[0:2] / (P @ Xh)[2:3] for P in P0])
    r = np.abs(proj - item["scene"].T).max(axis=0)
    return np.where(np.isfinite(r), r, 1e6)


def step(args, name, n_hyp):
    import torch
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.metrics import AngError_batch
    ctx = api.Context(0)
    items = load(name, args)
    S = len(items)
    packed, off = api.pack_ragged([it["scene"] for it in items])
    calms = np.stack([it["CalM"] for it in items])
    d_all = torch.from_numpy(packed).cuda(); d_off = torch.from_numpy(off).cuda(); d_calms = torch.from_numpy(calms).cuda()
    ns_max = int(np.diff(off).max())
    res_all = np.concatenate([residuals(ctx, it) for it in items])
    rng = np.random.default_rng(args.seed)
    orders = {"uniform": None}
    for label, sigma in SIGMAS:
        quality = -np.log1p(res_all) + rng.normal(0.0, sigma, res_all.shape[0])
        orders[label] = torch.from_numpy(api.order_from_quality(quality, off)).cuda()
    for method in METHODS:
        def call(label):
            more = {} if orders[label] is None else dict(order=orders[label], growth=args.growth)
            return ctx.robust_pose_scenes(method, d_all, d_off, d_calms, n_hyp, THR, seed=args.seed, ns_max=ns_max, candidates=args.candidates,
                                          lo_rounds=args.rounds, **more)
        times = {k: [] for k in orders}
        res = {}
        for rep in range(args.reps + 1):                                      # repetition 0 is the warm-up
            for label in orders:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[label] = call(label)
                torch.cuda.synchronize()
                if rep:
                    times[label].append(time.perf_counter() - t0)
        t_uniform = float(np.median(times["uniform"]))
        for label in orders:
            out = {k: v.cpu().numpy() for k, v in res[label].items()}
            ok = np.nonzero(out["status"] == 0)[0]
            rot = np.zeros(ok.size); tr = np.zeros(ok.size)
            for j, s in enumerate(ok):
                r2, t2 = AngError_batch(items[s]["R_t0"][0], out["R_t_2"][s][None]); r3, t3 = AngError_batch(items[s]["R_t0"][1], out["R_t_3"][s][None])
                rot[j] = 0.5 * (r2[0] + r3[0]); tr[j] = 0.5 * (t2[0] + t3[0])
            med = lambda a: float(np.median(a)) if a.size else None
            t = float(np.median(times[label]))
            line = {"tool": "bench_robust_guided", "quality": "synthetic: -log1p(ground-truth residual) + N(0, sigma)", "dataset": name, "scenes": S,
                    "n_hyp": n_hyp, "method": method, "sampler": label, "sigma": dict(SIGMAS).get(label), "growth": None if label == "uniform" else args.growth,
                    "threshold": THR, "candidates": args.candidates, "lo_rounds": args.rounds, "poses": int(ok.size),
                    "good_poses": int(((rot < GOOD[0]) & (tr < GOOD[1])).sum()), "rot_err_deg_median": med(rot), "t_err_deg_median": med(tr),
                    "inliers_total": int(out["inliers"][ok].sum()), "call_ms": 1e3 * t, "call_ms_min_max": [1e3 * min(times[label]), 1e3 * max(times[label])],
                    "overhead_vs_uniform": None if label == "uniform" else t / t_uniform - 1.0, "reps": args.reps}
            print(json.dumps(line), flush=True)


SAMPLER_SHAPES = ((400, 1000, 7), (400, 64000, 7), (1400, 150000, 7), (1400, 150000, 8))   # (Ns, rows, sample size)


def sampler_step(args):
    import torch
    from tft_vs_fund_amd import api
    ctx = api.Context(0)

    def timed(fn, reps=30):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}
    for Ns, B, n in SAMPLER_SHAPES:
        order = torch.from_numpy(np.random.default_rng(1).permutation(Ns).astype(np.int32)).cuda()
        print(json.dumps({"tool": "bench_robust_guided", "mode": "sampler-only", "Ns": Ns, "rows": B, "n_sample": n, "unit": "us, device time by events",
                          "uniform": timed(lambda: ctx.sample_indices(5, 0, B, n, Ns)),
                          "guided": timed(lambda: ctx.sample_indices_guided(5, 0, B, n, order, args.growth)),
                          "guided_growth_1": timed(lambda: ctx.sample_indices_guided(5, 0, B, n, order, 1))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", nargs="+", default=["fountain", "herzjesu", "synth50", "synth65"])
    ap.add_argument("--hyp", type=int, nargs="+", default=[64, 256, 1000])
    ap.add_argument("--growth", type=int, default=200000)
    ap.add_argument("--scenes", type=int, default=64, help="synthetic scenes per dataset")
    ap.add_argument("--matches", type=int, default=400, help="matches per synthetic scene")
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds a (dataset, n_hyp) step may take")
    ap.add_argument("--step", nargs=2, metavar=("DATASET", "N_HYP"), help="run this one step in this process (what the parent starts)")
    ap.add_argument("--sampler-only", action="store_true", help="time the guided sampler alone against the uniform one")
    ap.add_argument("--sampler-step", action="store_true", help="run the sampler measurement in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step[0], int(args.step[1]))
    if args.sampler_step:
        return sampler_step(args)
    if args.sampler_only:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--sampler-step", "--growth", str(args.growth)], timeout=args.step_timeout).returncode
        if rc != 0:
            sys.exit("the sampler measurement ended with status %d" % rc)
        return
    print("# the quality is SYNTHETIC: -log1p(ground-truth reprojection residual) + N(0, sigma), sigma = %s" % ", ".join("%g" % s for _, s in SIGMAS),
          flush=True)
    common = ["--growth", str(args.growth), "--scenes", str(args.scenes), "--matches", str(args.matches), "--candidates", str(args.candidates),
              "--rounds", str(args.rounds), "--reps", str(args.reps), "--seed", str(args.seed)]
    for name in args.datasets:
        for n_hyp in args.hyp:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(n_hyp)] + common, timeout=args.step_timeout).returncode
            if rc != 0:                                                       # nothing more is started on the GPU after a step that failed
                sys.exit("step %s at n_hyp = %d ended with status %d" % (name, n_hyp, rc))


if __name__ == "__main__":
    main()
