#!/usr/bin/env python3
"""
What stopping at a confidence costs and finds: Context.robust_pose_scenes over the fountain (150) and Herz-Jesu (56) triplet lists of
tests/golden/epfl_all.npz, LinearTFT and LinearF hypotheses, thresholds of 4 and 8 px, 16 candidates, two refit rounds, in three variants:

  fixed_1000   n_hyp = 1 000 for every triplet (the call as it was measured so far)
  fixed_cap    n_hyp = CAP for every triplet
  adaptive     cap CAP, confidence 0.99, first_round 256: every triplet stops once its best hypothesis allows it

CAP = 65 536.  The three are alternated in one process, each the median of `--reps` repetitions after a warm-up, host clock around a synchronise.  One JSON
line per dataset with, per (method, threshold, variant): ms per call [min, max], the triplets with a pose, median and 90th percentile over those of the
rotation and translation AngError against the EPFL ground truth (metrics.AngError_batch; per triplet the mean over views 2 and 3, degrees), and for the
adaptive variant the sum and median of n_hyp_used and the number of triplets that ran to the cap.

Each dataset runs in a child process under its own time limit; the first one that fails ends the run.

  python tools/bench_robust_adaptive.py [--datasets fountain herzjesu] [--methods tft f] [--thresholds 4 8] [--cap 65536] [--reps 7] [--step-timeout 600]
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

METHODS = {"tft": "LinearTFTPoseEstimation", "f": "LinearFPoseEstimation"}
VARIANTS = ("fixed_1000", "fixed_cap", "adaptive")


def step(args, name):
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
    rec = {"tool": "bench_robust_adaptive", "dataset": name, "triplets": S, "matches": int(off[-1]), "cap": args.cap, "confidence": args.confidence,
           "first_round": args.first_round, "candidates": args.candidates, "lo_rounds": args.rounds, "reps": args.reps, "results": []}
    for m in args.methods:
        method = METHODS[m]
        for thr in args.thresholds:
            kw = dict(seed=args.seed, ns_max=ns_max, candidates=args.candidates, lo_rounds=args.rounds)
            calls = {"fixed_1000": lambda: ctx.robust_pose_scenes(method, d_all, d_off, d_calms, 1000, thr, **kw),
                     "fixed_cap": lambda: ctx.robust_pose_scenes(method, d_all, d_off, d_calms, args.cap, thr, **kw),
                     "adaptive": lambda: ctx.robust_pose_scenes(method, d_all, d_off, d_calms, args.cap, thr, confidence=args.confidence,
                                                                first_round=args.first_round, **kw)}
            times = {v: [] for v in VARIANTS}
            res = {}
            for rep in range(args.reps + 1):                                  # repetition 0 is the warm-up
                for v in VARIANTS:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res[v] = calls[v]()
                    torch.cuda.synchronize()
                    if rep:
                        times[v].append(time.perf_counter() - t0)
            for v in VARIANTS:
                out = {k: a.cpu().numpy() for k, a in res[v].items()}
                ok = np.nonzero(out["status"] == 0)[0]
                rot = np.zeros(ok.size); tr = np.zeros(ok.size)
                for j, s in enumerate(ok):
                    r2, t2 = AngError_batch(trips[s]["R_t0"][0], out["R_t_2"][s][None]); r3, t3 = AngError_batch(trips[s]["R_t0"][1], out["R_t_3"][s][None])
                    rot[j] = 0.5 * (r2[0] + r3[0]); tr[j] = 0.5 * (t2[0] + t3[0])
                pct = lambda a, q: float(np.percentile(a, q)) if a.size else None
                t = times[v]
                r = {"method": method, "threshold": thr, "variant": v, "ms": 1e3 * float(np.median(t)), "ms_min_max": [1e3 * float(min(t)), 1e3 * float(max(t))],
                     "poses": int(ok.size), "inliers_total": int(out["inliers"][ok].sum()), "rot_err_deg": {"median": pct(rot, 50), "p90": pct(rot, 90)},
                     "t_err_deg": {"median": pct(tr, 50), "p90": pct(tr, 90)}}
                if v == "adaptive":
                    used = out["n_hyp_used"]
                    ran = used[used > 0]
                    r.update(n_hyp_used_sum=int(used.astype(np.int64).sum()), n_hyp_used_median=float(np.median(ran)) if ran.size else None,
                             at_cap=int((used == args.cap).sum()))
                rec["results"].append(r)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", nargs="+", default=["fountain", "herzjesu"])
    ap.add_argument("--methods", nargs="+", default=["tft", "f"], choices=sorted(METHODS))
    ap.add_argument("--thresholds", type=float, nargs="+", default=[4.0, 8.0])
    ap.add_argument("--cap", type=int, default=65536)
    ap.add_argument("--confidence", type=float, default=0.99)
    ap.add_argument("--first-round", type=int, default=256)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds a dataset may take")
    ap.add_argument("--step", metavar="DATASET", help="run this one dataset in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step)
    common = ["--methods"] + args.methods + ["--thresholds"] + [repr(t) for t in args.thresholds] + [
        "--cap", str(args.cap), "--confidence", repr(args.confidence), "--first-round", str(args.first_round), "--candidates", str(args.candidates),
        "--rounds", str(args.rounds), "--reps", str(args.reps), "--seed", str(args.seed)]
    for name in args.datasets:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name] + common, timeout=args.step_timeout).returncode
        if rc != 0:                                                           # nothing more is started on the GPU after a step that failed
            sys.exit("dataset %s ended with status %d" % (name, rc))


if __name__ == "__main__":
    main()
