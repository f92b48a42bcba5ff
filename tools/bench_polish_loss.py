#!/usr/bin/env python3
"""
What a robust loss in the polish of the robust estimators buys and costs (Context.robust_pose_scenes(..., polish=True, polish_loss=...),
Context.bundle_adjust_ragged(..., loss=...); include/tftfund_loss.h).

Accuracy: the fountain and Herz-Jesu triplet lists of tests/golden/epfl_all.npz, and 64 synthetic scenes of 400 matches after the recipe of
tools/config4_ransac.py (0.5 px noise, a share of the matches displaced by U(20, 80) px in views 2 and 3) at 30 % and 50 % displaced.  ONE robust call
per dataset (LinearTFT, threshold 4 px, --hyp hypotheses) gives the poses and the hard inlier mask; the polish then runs from those poses in four variants:
  mask            the hard mask, least squares (what polish=True does today)
  mask_cauchy     the hard mask, Cauchy at the threshold
  all_cauchy      all matches, Cauchy at the threshold
  all_huber       all matches, Huber at the threshold
Per variant: scenes polished with status 0, the median rotation / translation error against the ground truth (degrees, mean of views 2 and 3 per
scene, metrics.AngError_batch) over the scenes every variant polished, and ms per polish call (median of --reps after a warm-up, host clock around a
synchronise).  The errors of the unpolished robust poses are printed with the dataset.
Cost: the workload of tools/bench_ba_ragged.py (the whole list from LinearTFT starts, no mask), loss=None against Cauchy and Huber at 3 px, the
variants alternated in one process; and, to isolate an iteration's cost from the iteration counts, 256 clean synthetic scenes of one size through the
fixed-N call, ms per call over the iterations of the longest item.

Every (dataset, variant) step is a child process under its own time limit, and nothing more is started after a step that failed.  One JSON line per
step.  usage: python tools/bench_polish_loss.py [--datasets fountain herzjesu synth30 synth50] [--hyp 1000] [--reps 7] [--no-cost]
"""
import argparse, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

THR = 4.0
VARIANTS = {"mask": dict(), "mask_cauchy": dict(polish_loss="cauchy"), "all_cauchy": dict(polish_loss="cauchy", polish_all=True),
            "all_huber": dict(polish_loss="huber", polish_all=True)}
COST_SCALE = 3.0


def load(name, args):
    """-> list of dict(scene (n, 6), CalM (9, 3), R_t0 [2 x (3, 4)])"""
    if name in ("fountain", "herzjesu"):
        from tft_vs_fund_amd.experiments import load_epfl_all
        return [dict(scene=np.ascontiguousarray(t["Corresp"].T), CalM=t["CalM"], R_t0=t["R_t0"])
                for t in load_epfl_all(os.path.join(ROOT, "tests", "golden", "epfl_all.npz"), name)]
    from tft_vs_fund_amd.scenes import generate_scene_batch
    share = {"synth30": 0.30, "synth50": 0.50}[name]
    items = []
    for k in range(args.scenes):
        C, CalM, Rt0, _ = generate_scene_batch(1, args.matches, noise=0.5, seed=7 + k)
        scene = C[0].copy()
        rng = np.random.default_rng(1 + k)
        bad = rng.choice(args.matches, int(share * args.matches), replace=False)
        scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
        items.append(dict(scene=np.ascontiguousarray(scene), CalM=np.ascontiguousarray(CalM), R_t0=Rt0))
    return items


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def step(args, name, variant):
    import torch
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.metrics import AngError_batch
    ctx = api.Context(0)
    items = load(name, args)
    S = len(items)
    packed, off = api.pack_ragged([it["scene"] for it in items])
    pk, of, calm = torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(np.stack([it["CalM"] for it in items])).cuda()
    rob = ctx.robust_pose_scenes("LinearTFTPoseEstimation", pk, of, calm, args.hyp, THR, seed=args.seed, ns_max=int(np.diff(off).max()))
    loss, over_all = VARIANTS[variant].get("polish_loss"), VARIANTS[variant].get("polish_all", False)

    def errors(R2, R3, ok):
        R2, R3 = R2.cpu().numpy(), R3.cpu().numpy()
        e = np.full((S, 2), np.nan)
        for s in np.nonzero(ok)[0]:
            r2, t2 = AngError_batch(items[s]["R_t0"][0], R2[s][None]); r3, t3 = AngError_batch(items[s]["R_t0"][1], R3[s][None])
            e[s] = (float(r2[0]) + float(r3[0])) / 2, (float(t2[0]) + float(t3[0])) / 2
        return e

    def polish():                                                             # what robust_pose_scenes(..., polish=True, **VARIANTS[variant]) adds to the robust call
        return ctx.bundle_adjust_ragged(calm, rob["R_t_2"], rob["R_t_3"], pk, of, mask=None if over_all else rob["mask"], reconst=False, loss=loss,
                                        scale=None if loss is None else THR)

    out = polish()
    torch.cuda.synchronize()
    times = [timed(torch, polish) for _ in range(args.reps)]
    ok0 = rob["status"].cpu().numpy() == 0
    ok = ok0 & (out["status"].cpu().numpy() == 0)
    e0, e1 = errors(rob["R_t_2"], rob["R_t_3"], ok0), errors(out["R_t_2"], out["R_t_3"], ok)
    line = {"tool": "bench_polish_loss", "dataset": name, "variant": variant, "scenes": S, "n_hyp": args.hyp, "threshold": THR, "with_pose": int(ok0.sum()),
            "polished": int(ok.sum()), "iter_median": float(np.median(out["iter"].cpu().numpy()[ok])) if ok.any() else None,
            "ms": {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times))},
            "rot_err": e1[:, 0].tolist(), "trans_err": e1[:, 1].tolist(), "rot_err_robust": e0[:, 0].tolist(), "trans_err_robust": e0[:, 1].tolist()}
    if "weight" in out:
        w, m = out["weight"].cpu().numpy(), rob["mask"].cpu().numpy() != 0
        line["weight_median_inliers"] = float(np.nanmedian(w[m])) if m.any() else None
        if over_all:
            line["weight_median_outliers"] = float(np.nanmedian(w[~m])) if (~m).any() else None
    print(json.dumps(line), flush=True)


def cost_step(args):
    import torch
    from tft_vs_fund_amd import api
    d = np.load(os.path.join(ROOT, "tests", "golden", "epfl_all.npz"))
    ctx = api.Context(0)
    for name in ("fountain", "herzjesu"):
        off, K, trip = d[name + "_offsets"], d[name + "_K"], d[name + "_triplets"]
        S = off.shape[0] - 1
        calms = np.stack([np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0) for t in range(S)])
        packed = torch.from_numpy(np.ascontiguousarray(d[name + "_corresp"])).cuda()
        lin = ctx.pose_batch_ragged("LinearTFTPoseEstimation", packed, torch.from_numpy(off).cuda(), torch.from_numpy(calms).cuda(), reconst=True,
                                    n_max=int(np.diff(off).max()))
        ok = np.nonzero(lin["status"].cpu().numpy() == 0)[0]
        pk, o2 = api.pack_ragged([d[name + "_corresp"][off[t]:off[t + 1]] for t in ok])
        pk_d, off_d, calm_d = torch.from_numpy(pk).cuda(), torch.from_numpy(o2).cuda(), torch.from_numpy(calms[ok]).cuda()
        sel = torch.from_numpy(ok).cuda()
        r2, r3 = lin["R_t_2"][sel].contiguous(), lin["R_t_3"][sel].contiguous()
        calls = {"none": lambda: ctx.bundle_adjust_ragged(calm_d, r2, r3, pk_d, off_d),
                 "cauchy": lambda: ctx.bundle_adjust_ragged(calm_d, r2, r3, pk_d, off_d, loss="cauchy", scale=COST_SCALE),
                 "huber": lambda: ctx.bundle_adjust_ragged(calm_d, r2, r3, pk_d, off_d, loss="huber", scale=COST_SCALE)}
        outs = {k: f() for k, f in calls.items()}                             # warm-up
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, f in calls.items():
                times[k].append(timed(torch, f))
        it = {k: outs[k]["iter"].cpu().numpy() for k in calls}
        st = {k: outs[k]["status"].cpu().numpy() for k in calls}
        print(json.dumps({"tool": "bench_polish_loss", "cost": name, "triplets": int(ok.size), "scale": COST_SCALE,
                          "ms": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in times.items()},
                          "iter_sum": {k: int(it[k].sum()) for k in calls}, "iter_max": {k: int(it[k].max()) for k in calls},
                          "bad_status": {k: int((st[k] != 0).sum()) for k in calls}}), flush=True)


def unit_cost_step(args):
    """the cost of an iteration: 256 clean synthetic scenes of one size (no displaced matches, 0.5 px noise), starts from LinearTFT, so that every item
    runs the same few iterations and a call lasts as long as iter_max of them; ms per call over iter_max, per variant, alternated in one process"""
    import torch
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.scenes import generate_scene_batch
    ctx = api.Context(0)
    B, N = 256, args.matches
    C, CalM, _, _ = generate_scene_batch(B, N, noise=0.5, seed=99)
    Cd, calm = torch.from_numpy(np.ascontiguousarray(C)).cuda(), torch.from_numpy(np.ascontiguousarray(CalM)).cuda()
    lin = ctx.pose_batch("LinearTFTPoseEstimation", Cd, calm, reconst=False)
    r2, r3 = lin["R_t_2"].contiguous(), lin["R_t_3"].contiguous()
    calls = {"none": lambda: ctx.bundle_adjust(calm, r2, r3, Cd), "cauchy": lambda: ctx.bundle_adjust(calm, r2, r3, Cd, loss="cauchy", scale=COST_SCALE),
             "huber": lambda: ctx.bundle_adjust(calm, r2, r3, Cd, loss="huber", scale=COST_SCALE)}
    outs = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, f in calls.items():
            times[k].append(timed(torch, f))
    it = {k: outs[k]["iter"].cpu().numpy() for k in calls}
    print(json.dumps({"tool": "bench_polish_loss", "unit_cost": "%d clean scenes x %d matches" % (B, N), "scale": COST_SCALE,
                      "ms": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in times.items()},
                      "iter_max": {k: int(it[k].max()) for k in calls}, "iter_min": {k: int(it[k].min()) for k in calls},
                      "bad_status": {k: int((outs[k]["status"] != 0).sum()) for k in calls},
                      "ms_per_iteration_of_the_longest_item": {k: float(np.median(times[k]) / max(1, int(it[k].max()))) for k in calls}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", nargs="+", default=["fountain", "herzjesu", "synth30", "synth50"])
    ap.add_argument("--hyp", type=int, default=1000)
    ap.add_argument("--scenes", type=int, default=64, help="synthetic scenes per dataset")
    ap.add_argument("--matches", type=int, default=400, help="matches per synthetic scene")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--no-cost", action="store_true")
    ap.add_argument("--step", nargs=2, metavar=("DATASET", "VARIANT"), help="run this one step in this process (what the parent starts)")
    ap.add_argument("--cost-step", action="store_true", help="run the cost measurement in this process (what the parent starts)")
    ap.add_argument("--unit-cost-step", action="store_true", help="run the per-iteration cost measurement in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step[0], args.step[1])
    if args.cost_step:
        return cost_step(args)
    if args.unit_cost_step:
        return unit_cost_step(args)
    common = ["--hyp", str(args.hyp), "--scenes", str(args.scenes), "--matches", str(args.matches), "--reps", str(args.reps), "--seed", str(args.seed)]
    table = []
    for name in args.datasets:
        lines = {}
        for variant in VARIANTS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, variant] + common, timeout=args.step_timeout, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:                                             # nothing more is started on the GPU after a step that failed
                sys.exit("step %s / %s ended with status %d" % (name, variant, r.returncode))
            lines[variant] = json.loads(r.stdout.strip().splitlines()[-1])
        both = np.all([np.isfinite(np.array(l["rot_err"], dtype=float)) for l in lines.values()], axis=0)     # the scenes every variant polished
        base = lines["mask"]
        rob = (np.array(base["rot_err_robust"], dtype=float), np.array(base["trans_err_robust"], dtype=float))
        for variant, l in lines.items():
            l["common_scenes"] = int(both.sum())
            l["rot_err_median"] = float(np.median(np.array(l["rot_err"], dtype=float)[both])) if both.any() else None
            l["trans_err_median"] = float(np.median(np.array(l["trans_err"], dtype=float)[both])) if both.any() else None
            l["robust_rot_err_median"] = float(np.median(rob[0][both])) if both.any() else None
            l["robust_trans_err_median"] = float(np.median(rob[1][both])) if both.any() else None
            for k in ("rot_err", "trans_err", "rot_err_robust", "trans_err_robust"):
                del l[k]
            print(json.dumps(l), flush=True)
            table.append(l)
    if not args.no_cost:
        for flag in ("--cost-step", "--unit-cost-step"):
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), flag, "--reps", str(args.reps), "--matches", str(args.matches)],
                                timeout=args.step_timeout).returncode
            if rc != 0:
                sys.exit("the cost measurement %s ended with status %d" % (flag, rc))
    print("# dataset variant polished/common rot_med trans_med (robust rot_med trans_med) ms")
    for l in table:
        print("# %-9s %-12s %3d/%3d  %.3f %.3f  (%.3f %.3f)  %.2f" % (l["dataset"], l["variant"], l["polished"], l["common_scenes"], l["rot_err_median"] or -1,
                                                                    l["trans_err_median"] or -1, l["robust_rot_err_median"] or -1, l["robust_trans_err_median"] or -1,
                                                                    l["ms"]["median"]))


if __name__ == "__main__":
    main()
