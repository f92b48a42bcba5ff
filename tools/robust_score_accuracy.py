#!/usr/bin/env python3
"""
What the score of the robust estimators does to the pose and what it costs: Context.robust_pose_scenes over the fountain (150) and Herz-Jesu (56) triplet
lists of tests/golden/epfl_all.npz, LinearTFT hypotheses, 1 000 per triplet, 16 candidates, two refit rounds, with the inlier count
(set_score("count")) and with the MSAC score (set_score("msac")) at thresholds of 1, 2, 4 and 8 px, against the EPFL ground-truth poses.

One JSON line per (dataset, threshold, score): median and 90th percentile over the triplets with a pose of the rotation and translation AngError
(metrics.py; per triplet the mean over views 2 and 3, degrees), the number of triplets with a pose, the inliers in total, and the call time: the median of
`--reps` calls, the two scores alternated in one process after a warm-up call of each, host clock around a synchronise (as tools/bench_robust_scenes.py).

Each (dataset, threshold) step is a child process under its own time limit; the first step that fails ends the run.

  python tools/robust_score_accuracy.py [--datasets fountain herzjesu] [--thresholds 1 2 4 8] [--hyp 1000] [--reps 7] [--step-timeout 240]
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

METHOD = "LinearTFTPoseEstimation"
SCORES = ("count", "msac")


def step(args, name, thr):
    import torch
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.experiments import load_epfl_all
    from tft_vs_fund_amd.metrics import AngError_batch
    ctx = api.Context(0)
    trips = load_epfl_all(os.path.join(ROOT, "tests", "golden", "epfl_all.npz"), name)
    S = len(trips)
    packed, off = api.pack_ragged([np.ascontiguousarray(t["Corresp"].T) for t in trips])
    calms = np.stack([t["CalM"] for t in trips])
    d_all = torch.from_numpy(packed).cuda(); d_off = torch.from_numpy(off).cuda(); d_calms = torch.from_numpy(calms).cuda()
    ns_max = int(np.diff(off).max())

    def call(score):
        ctx.set_score(score)
        return ctx.robust_pose_scenes(METHOD, d_all, d_off, d_calms, args.hyp, thr, seed=args.seed, ns_max=ns_max, candidates=args.candidates,
                                      lo_rounds=args.rounds)
    times = {s: [] for s in SCORES}
    res = {}
    for rep in range(args.reps + 1):                                          # repetition 0 is the warm-up
        for score in SCORES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[score] = call(score)
            torch.cuda.synchronize()
            if rep:
                times[score].append(time.perf_counter() - t0)
    for score in SCORES:
        out = {k: v.cpu().numpy() for k, v in res[score].items()}
        ok = np.nonzero(out["status"] == 0)[0]
        rot = np.zeros(ok.size); tr = np.zeros(ok.size)
        for j, s in enumerate(ok):
            r2, t2 = AngError_batch(trips[s]["R_t0"][0], out["R_t_2"][s][None]); r3, t3 = AngError_batch(trips[s]["R_t0"][1], out["R_t_3"][s][None])
            rot[j] = 0.5 * (r2[0] + r3[0]); tr[j] = 0.5 * (t2[0] + t3[0])
        pct = lambda a, q: float(np.percentile(a, q)) if a.size else None
        t = times[score]
        print(json.dumps({"tool": "robust_score_accuracy", "dataset": name, "threshold": thr, "score": score, "method": METHOD, "triplets": S,
                          "hyp": args.hyp, "candidates": args.candidates, "lo_rounds": args.rounds, "poses": int(ok.size),
                          "inliers_total": int(out["inliers"][ok].sum()), "rot_err_deg": {"median": pct(rot, 50), "p90": pct(rot, 90)},
                          "t_err_deg": {"median": pct(tr, 50), "p90": pct(tr, 90)}, "call_seconds": float(np.median(t)),
                          "call_min_max": [float(min(t)), float(max(t))], "reps": args.reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", nargs="+", default=["fountain", "herzjesu"])
    ap.add_argument("--thresholds", type=float, nargs="+", default=[1.0, 2.0, 4.0, 8.0])
    ap.add_argument("--hyp", type=int, default=1000)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a (dataset, threshold) step may take")
    ap.add_argument("--step", nargs=2, metavar=("DATASET", "THRESHOLD"), help="run this one step in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step[0], float(args.step[1]))
    common = ["--hyp", str(args.hyp), "--candidates", str(args.candidates), "--rounds", str(args.rounds), "--reps", str(args.reps), "--seed", str(args.seed)]
    for name in args.datasets:
        for thr in args.thresholds:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, repr(thr)] + common, timeout=args.step_timeout).returncode
            if rc != 0:                                                       # nothing more is started on the GPU after a step that failed
                sys.exit("step %s at %g px ended with status %d" % (name, thr, rc))


if __name__ == "__main__":
    main()
