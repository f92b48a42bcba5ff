#!/usr/bin/env python3
"""
Robust pose estimation against the composition it replaces, on the config-4 scene (400 correspondences at 0.5 px noise, 100 of them displaced
by U(20, 80) px in views 2 and 3):

  (a) Context.robust_pose (tff_robust_pose_dev: capi.hip::robust_dev, the scene-list chain with S = 1): device-side sampler, hypotheses, counts,
      top-K selection, K refits per round -- one call, no host synchronisation;
  (b) what tools/config4_ransac.py times: torch sampler (rand + argsort) + pose_sampled + inlier_count + argmax.

Both at the same threshold, alternated in one process, each the median of `--reps` repetitions after a warm-up, timed with the host clock around
work that ends in a synchronise.  One JSON line.

  timeout 600 python tools/robust_bench.py [--hyp 1000000] [--method tft|f] [--threshold 4] [--reps 7]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hyp", type=int, default=1000000)
    ap.add_argument("--method", default="tft")
    ap.add_argument("--threshold", type=float, default=4.0)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.metrics import AngError_batch
    from tft_vs_fund_amd.scenes import generate_scene_batch
    ctx = api.Context(0)
    C, CalM, Rt0, _ = generate_scene_batch(1, 400, noise=0.5, seed=7)
    scene = C[0].copy()
    rng = np.random.default_rng(1)
    bad = rng.choice(400, 100, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    method = "LinearTFTPoseEstimation" if args.method == "tft" else "LinearFPoseEstimation"
    n = api.ROBUST_METHODS[method]
    d_scene = torch.from_numpy(scene).cuda(); d_calm = torch.from_numpy(CalM).cuda()
    g = torch.Generator(device="cuda"); g.manual_seed(args.seed)

    def robust():
        return ctx.robust_pose(method, d_scene, d_calm, args.hyp, args.threshold, seed=args.seed, candidates=args.candidates, lo_rounds=args.rounds)

    def composed():
        idx = torch.rand((args.hyp, 400), device="cuda", generator=g).argsort(dim=1)[:, :n].to(torch.int32).contiguous()
        hyp = ctx.pose_sampled(method, d_scene, d_calm, idx)
        cnt = ctx.inlier_count(d_scene, d_calm, hyp["R_t_2"], hyp["R_t_3"], args.threshold)
        return cnt, int(cnt.argmax())

    times = {"robust": [], "composed": []}
    out = best = None
    for rep in range(args.reps + 1):                                          # repetition 0 is the warm-up
        for name, fn in (("robust", robust), ("composed", composed)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
            if name == "robust":
                out = res
            else:
                best = int(res[0][res[1]])
    ta, tb = float(np.median(times["robust"])), float(np.median(times["composed"]))
    r2, t2 = AngError_batch(Rt0[0], out["R_t_2"].cpu().numpy()[None]); r3, t3 = AngError_batch(Rt0[1], out["R_t_3"].cpu().numpy()[None])
    mask = out["mask"].cpu().numpy() != 0
    print(json.dumps({"tool": "robust_bench", "method": method, "hypotheses": args.hyp, "threshold": args.threshold, "candidates": args.candidates,
                      "lo_rounds": args.rounds, "reps": args.reps, "robust_seconds": ta, "robust_hypotheses_per_s": args.hyp / ta,
                      "composed_seconds": tb, "composed_hypotheses_per_s": args.hyp / tb, "inliers": int(out["inliers"]),
                      "displaced_in_mask": int(mask[bad].sum()), "refits": int(out["refits"]), "composed_best_inliers": best,
                      "rot_err_deg": 0.5 * float(r2[0] + r3[0]), "t_err_deg": 0.5 * float(t2[0] + t3[0])}))


if __name__ == "__main__":
    main()
