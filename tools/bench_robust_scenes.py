#!/usr/bin/env python3
"""
Robust pose estimation over the triplet list of a dataset (tests/golden/epfl_all.npz: fountain, 150 triplets of 1 .. 1 400 matches with a CalM per
triplet; Herz-Jesu, 56 triplets), 4 px threshold, n_hyp hypotheses per triplet:

  (a) ONE Context.robust_pose_scenes call over the whole list;
  (b) the loop of Context.robust_pose over the same triplets on the same context (scene s with seed + s; triplets with fewer matches than a
      sample are skipped by the loop -- the batch call reports them ST_TOO_FEW).

The two are alternated in one process, each the median of `--reps` repetitions after a warm-up, timed with the host clock around work that ends in a
synchronise.  One JSON line per dataset; the results of (a) and (b) are compared bit for bit on the way (`equal`).
--refine NAME adds the refine step to both: `refine=NAME` in the one call (ONE ragged call of that method on every triplet's inliers) against
`refine=NAME` in every call of the loop (a fixed-N call per triplet, after reading its inlier count on the host); the loop then runs over the triplets
the batch call found a pose with inliers for, the refined outputs join the comparison, and `refine_seconds` is the difference to the same run without the step.

  timeout 900 python tools/bench_robust_scenes.py [--hyp 1000 10000] [--method tft|f] [--threshold 4] [--reps 7] [--datasets fountain herzjesu]
                                                  [--refine OptimFPoseEstimation]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hyp", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--method", default="tft")
    ap.add_argument("--threshold", type=float, default=4.0)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--datasets", nargs="+", default=["fountain", "herzjesu"])
    ap.add_argument("--refine", default=None, help="a method with a ragged route (api.RAGGED_METHODS): adds the refine step to both sides")
    args = ap.parse_args()
    from tft_vs_fund_amd import api
    ctx = api.Context(0)
    method = "LinearTFTPoseEstimation" if args.method == "tft" else "LinearFPoseEstimation"
    n = api.ROBUST_METHODS[method]
    d = np.load(os.path.join(ROOT, "tests", "golden", "epfl_all.npz"))
    kw = dict(candidates=args.candidates, lo_rounds=args.rounds)
    for name in args.datasets:
        off = d[name + "_offsets"]; K = d[name + "_K"]; trip = d[name + "_triplets"]
        S = off.shape[0] - 1
        calms = np.stack([np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0) for t in range(S)])
        d_all = torch.from_numpy(np.ascontiguousarray(d[name + "_corresp"])).cuda()
        d_off = torch.from_numpy(off).cuda()
        d_calms = torch.from_numpy(calms).cuda()
        sizes = np.diff(off)
        ns_max = int(sizes.max())
        views = [(s, d_all[off[s]:off[s + 1]], d_calms[s]) for s in range(S) if sizes[s] >= n]
        rec = {"tool": "bench_robust_scenes", "dataset": name, "method": method, "triplets": S, "matches": int(off[-1]), "looped_triplets": len(views),
               "threshold": args.threshold, "candidates": args.candidates, "lo_rounds": args.rounds, "reps": args.reps}
        if args.refine:
            rec["refine"] = args.refine
        for n_hyp in args.hyp:
            looped = views
            if args.refine:                                                   # (the one-scene call has nothing to refine on where there is no pose or no inlier)
                first = ctx.robust_pose_scenes(method, d_all, d_off, d_calms, n_hyp, args.threshold, seed=args.seed, ns_max=ns_max, **kw)
                st, inl = first["status"].cpu().numpy(), first["inliers"].cpu().numpy()
                looped = [v for v in views if st[v[0]] == 0 and inl[v[0]] > 0]

            def batch(refine=args.refine):
                return ctx.robust_pose_scenes(method, d_all, d_off, d_calms, n_hyp, args.threshold, seed=args.seed, ns_max=ns_max, refine=refine, **kw)

            def loop(refine=args.refine):
                return [(s, ctx.robust_pose(method, sc, cm, n_hyp, args.threshold, seed=args.seed + s, refine=refine, **kw)) for s, sc, cm in looped]

            runs = [("batch", batch), ("loop", loop)]
            if args.refine:
                runs += [("batch_plain", lambda: batch(None)), ("loop_plain", lambda: loop(None))]
            times = {what: [] for what, _ in runs}
            res = {}
            for rep in range(args.reps + 1):                                  # repetition 0 is the warm-up
                for what, fn in runs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res[what] = fn()
                    torch.cuda.synchronize()
                    if rep:
                        times[what].append(time.perf_counter() - t0)
            a = {k: v.cpu().numpy() for k, v in res["batch"].items()}
            equal = True
            for s, o in res["loop"]:
                equal = equal and int(o["status"]) == int(a["status"][s]) and int(o["inliers"]) == int(a["inliers"][s])
                equal = equal and np.array_equal(o["mask"].cpu().numpy(), a["mask"][off[s]:off[s + 1]])
                for k in ("R_t_2", "R_t_3", "T") + (("R_t_2_refined", "R_t_3_refined", "T_refined") if args.refine else ()):
                    equal = equal and np.array_equal(np.ascontiguousarray(o[k].cpu().numpy()).view(np.int64), np.ascontiguousarray(a[k][s]).view(np.int64))
            ta, tb = float(np.median(times["batch"])), float(np.median(times["loop"]))
            rec["hyp_%d" % n_hyp] = {"scenes_call_seconds": ta, "loop_seconds": tb, "loop_over_scenes_call": tb / ta,
                                     "scenes_call_min_max": [float(min(times["batch"])), float(max(times["batch"]))],
                                     "loop_min_max": [float(min(times["loop"])), float(max(times["loop"]))],
                                     "poses": int((a["status"] == 0).sum()), "inliers_total": int(a["inliers"].sum()), "equal": bool(equal)}
            if args.refine:
                pa, pb = float(np.median(times["batch_plain"])), float(np.median(times["loop_plain"]))
                rec["hyp_%d" % n_hyp].update(looped_triplets=len(looped), refine_seconds={"scenes_call": ta - pa, "loop": tb - pb},
                                             refined_ok=int((a["status_refined"] == 0).sum()), iter_refined_total=int(a["iter_refined"].sum()))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
