"""What does the covariance of a bundle adjustment over tracks cost?

Windows of M = 4, 5, 6 consecutive views of fountain-P11 and Herz-Jesu-P8 (tests/golden/epfl_all.npz), tracks merged and filtered at 1 px as
tools/bench_ba_tracks.py does (tests/ba_tracks_cases.window_tracks), every window started from the ground-truth poses perturbed by a fixed seed, at most
--max-tracks tracks of a window kept by a fixed seed (the adjustment keeps its points in LDS), all windows of one M in ONE call padded with NaN
columns.  Three calls on the same input in the same process, alternated, host clock around a synchronise, median of --reps (7) after a warm-up:
  adjust        Context.bundle_adjust_views(missing="point")                       tff_bundle_adjust_tracks_batch_dev, the kernel of the parent commit
  adjust_cov    ... with cov=True, point_cov=True                                  tff_bundle_adjust_tracks_cov_batch_dev
  cov           Context.ba_tracks_covariance(point_cov=True) on adjust's outputs   tff_ba_tracks_covariance_batch_dev
cov_share = (adjust_cov - adjust) / adjust_cov: the share of the combined call that the covariance takes; the comparison is the same run's call without
a covariance.  The three calls again under --loss cauchy at --scale (3 px).  sigma0_median and the median standard deviation of a rotation in degrees
(api.euler_cov_to_rotvec_views) say what the numbers are good for.
Each M runs in a child process under its own time limit (--limit seconds); the first child that fails or runs out of time ends the run.
Prints one JSON line per M, then one summary line.  usage: python tools/bench_ba_tracks_cov.py [--reps 7] [--max-tracks 2000] [--scale 3] [--limit 300]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS, MAX_TRACKS, LIMIT, SCALE = arg("--reps", 7), arg("--max-tracks", 2000), arg("--limit", 300), arg("--scale", 3.0, float)
IMAGES = {"fountain": 11, "herzjesu": 8}


def windows(M):
    import ba_tracks_cases as tc
    out = []
    for ds, n_img in IMAGES.items():
        for first in range(1, n_img - M + 2):
            C, CalM, R_t, _ = tc.window_tracks(ds, first, M, max_px=1.0)
            rng = np.random.default_rng(1000 * M + first)
            if C.shape[1] > MAX_TRACKS:
                C = np.ascontiguousarray(C[:, np.sort(rng.permutation(C.shape[1])[:MAX_TRACKS])])
            out.append(dict(name="%s %d..%d" % (ds, first, first + M - 1), C=C, CalM=CalM, R0=tc._perturbed(R_t, rng)))
    return out


def worker(M):
    import torch
    from tft_vs_fund_amd import api
    ctx = api.Context(0)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ws = windows(M)
    n = max(w["C"].shape[1] for w in ws)
    inp = (cu(np.stack([w["CalM"] for w in ws])), cu(np.stack([w["R0"] for w in ws])),
           cu(np.stack([np.hstack([w["C"], np.full((2 * M, n - w["C"].shape[1]), np.nan)]).T for w in ws])))
    res = {"tracks": [int(w["C"].shape[1]) for w in ws]}
    for name, kw in (("none", {}), ("cauchy", dict(loss="cauchy", scale=SCALE))):
        o = ctx.bundle_adjust_views(*inp, missing="point", **kw); torch.cuda.synchronize()
        R_t, X = o["R_t"].contiguous(), o["Reconst"].contiguous()
        ways = {"adjust": lambda: ctx.bundle_adjust_views(*inp, missing="point", **kw),
                "adjust_cov": lambda: ctx.bundle_adjust_views(*inp, missing="point", cov=True, point_cov=True, **kw),
                "cov": lambda: ctx.ba_tracks_covariance(inp[0], R_t, inp[2], X, point_cov=True, **kw)}
        both = ways["adjust_cov"](); alone = ways["cov"](); torch.cuda.synchronize()   # results and warm-up
        cov = both["cov"].cpu().numpy(); s0 = both["sigma0"].cpu().numpy()
        ok = np.isfinite(s0)
        rv = api.euler_cov_to_rotvec_views(both["R_t"].cpu().numpy()[ok], cov[ok])
        rot_sd = np.degrees(np.sqrt(np.array([[np.trace(q[3 * j:3 * j + 3, 3 * j:3 * j + 3]) for j in range(M - 1)] for q in rv])))
        r = dict(bad_status=int((o["status"] != 0).sum()), iter_sum=int(o["iter"].sum()), nan_cov=int((~ok).sum()), sigma0_median=float(np.median(s0[ok])),
                 rot_sd_deg_median=float(np.median(rot_sd)), same_bits=bool(np.array_equal(cov[ok].view(np.int64), alone["cov"].cpu().numpy()[ok].view(np.int64))))
        times = {k: [] for k in ways}
        for _ in range(REPS):                                                            # alternated
            for k, f in ways.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                f()
                torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
        for k in ways:
            r[k] = dict(ms=float(np.median(times[k])), ms_min=float(np.min(times[k])), ms_max=float(np.max(times[k])))
        r["cov_share"] = (r["adjust_cov"]["ms"] - r["adjust"]["ms"]) / r["adjust_cov"]["ms"]
        res[name] = r
    print(json.dumps({"tool": "bench_ba_tracks_cov", "M": M, "windows": len(ws), "n_padded": n, "reps": REPS, "max_tracks": MAX_TRACKS, "scale": SCALE, **res}))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(arg("--worker", 4))
        sys.exit(0)
    lines = []
    for M in (4, 5, 6):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(M), "--reps", str(REPS), "--max-tracks", str(MAX_TRACKS), "--scale", str(SCALE)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print("M = %d did not finish in %d s: stopping" % (M, LIMIT)); sys.exit(124)
        if r.returncode != 0:
            print("M = %d failed with status %d: stopping" % (M, r.returncode)); sys.exit(1)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        lines.append(json.loads(line))
    print(json.dumps({"tool": "bench_ba_tracks_cov", "summary": [
        {"M": l["M"], "windows": l["windows"], "n_padded": l["n_padded"],
         **{k + "_ms": [round(l[k][w]["ms"], 3) for w in ("adjust", "adjust_cov", "cov")] for k in ("none", "cauchy")},
         **{k + "_cov_share": round(l[k]["cov_share"], 3) for k in ("none", "cauchy")}} for l in lines]}))
