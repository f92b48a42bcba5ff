"""What does a robust loss per observation buy on raw tracks, and what does it cost?

Windows of M = 4, 5, 6 consecutive views of fountain-P11 and Herz-Jesu-P8 (tests/golden/epfl_all.npz), tracks merged as tools/bench_ba_tracks.py merges
them (tests/ba_tracks_cases.window_tracks), every window started from the ground-truth poses perturbed by a fixed seed, all windows of one M in ONE call
padded with NaN columns.  Two regimes:
  raw       the tracks WITHOUT the <= 1 px ground-truth filter (--max-px inf; a finite value filters at that many pixels -- say so where it is used), at
            most --max-tracks tracks of a window kept by a fixed seed (the points live in LDS): plain tracks, Huber and Cauchy at --scale (3 px).  Median
            and worst rotation / translation error of the cameras 2 .. M against the ground truth, iter, ms per call.
  filtered  the <= 1 px tracks of DESIGN 3.4 through the plain kernel and through a loss instance at c = 1e6 px, where every weight is 1: the loss's cost
            per iteration, apart from the iterations it adds (per_iteration_ratio = (ms / sum of iter) of the loss instance over that of the plain one).
Timing: the plain call (k_bundle_adjust_tracks, the kernel of the parent commit) and the loss calls on the same input in the same process, alternated,
host clock around a synchronise, median of --reps (7) after a warm-up.
Each M runs in a child process under its own time limit (--limit seconds); the first child that fails or runs out of time ends the run.
Prints one JSON line per M, then one summary line.  usage: python tools/bench_ba_tracks_loss.py [--reps 7] [--max-tracks 2000] [--max-px inf] [--scale 3] [--limit 300]"""
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


REPS, MAX_TRACKS, LIMIT = arg("--reps", 7), arg("--max-tracks", 2000), arg("--limit", 300)
MAX_PX, SCALE = arg("--max-px", float("inf"), float), arg("--scale", 3.0, float)
IMAGES = {"fountain": 11, "herzjesu": 8}


def windows(M, max_px):
    import ba_tracks_cases as tc
    out = []
    for ds, n_img in IMAGES.items():
        for first in range(1, n_img - M + 2):
            C, CalM, R_t, _ = tc.window_tracks(ds, first, M, max_px=max_px)
            rng = np.random.default_rng(1000 * M + first)
            if C.shape[1] > MAX_TRACKS:
                C = np.ascontiguousarray(C[:, np.sort(rng.permutation(C.shape[1])[:MAX_TRACKS])])
            G = np.vstack([R_t[0:3], [0, 0, 0, 1]])
            out.append(dict(name="%s %d..%d" % (ds, first, first + M - 1), C=C, CalM=CalM, R0=tc._perturbed(R_t, rng),
                            truth=[R_t[3 * j:3 * j + 3] @ np.linalg.inv(G) for j in range(1, M)]))     # cameras 2 .. M in the frame of camera 1
    return out


def worker(M):
    import torch
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.metrics import AngError_batch
    ctx = api.Context(0)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def regime(ws, ways):
        n = max(w["C"].shape[1] for w in ws)
        inp = (cu(np.stack([w["CalM"] for w in ws])), cu(np.stack([w["R0"] for w in ws])),
               cu(np.stack([np.hstack([w["C"], np.full((2 * M, n - w["C"].shape[1]), np.nan)]).T for w in ws])))
        res = {}
        for k, kw in ways.items():                                                       # results and warm-up
            o = ctx.bundle_adjust_views(*inp, missing="point", **kw); torch.cuda.synchronize()
            R = o["R_t"].cpu().numpy(); it = o["iter"].cpu().numpy(); st = o["status"].cpu().numpy()
            rot, tr = [], []
            for b, w in enumerate(ws):
                for j in range(1, M):
                    r, t = AngError_batch(w["truth"][j - 1], R[b:b + 1, 3 * j:3 * j + 3])
                    rot.append(float(r[0])); tr.append(float(t[0]))
            res[k] = dict(rot_deg_median=float(np.nanmedian(rot)), rot_deg_max=float(np.nanmax(rot)), t_deg_median=float(np.nanmedian(tr)), t_deg_max=float(np.nanmax(tr)),
                          bad_status=int((st != 0).sum()), iter_median=float(np.median(it)), iter_max=int(it.max()), iter_sum=int(it.sum()))
            if "weight" in o:
                wt = o["weight"].cpu().numpy()
                res[k]["weight_below_0.1"] = float((wt[np.isfinite(wt)] < 0.1).mean())
        times = {k: [] for k in ways}
        for _ in range(REPS):                                                            # alternated
            for k, kw in ways.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                ctx.bundle_adjust_views(*inp, missing="point", **kw)
                torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
        for k in ways:
            res[k].update(ms=float(np.median(times[k])), ms_min=float(np.min(times[k])), ms_max=float(np.max(times[k])))
        res["tracks"] = [int(w["C"].shape[1]) for w in ws]
        return res

    raw = regime(windows(M, MAX_PX), {"plain": {}, "huber": dict(loss="huber", scale=SCALE), "cauchy": dict(loss="cauchy", scale=SCALE)})
    flt = regime(windows(M, 1.0), {"plain": {}, "huber_1e6": dict(loss="huber", scale=1e6)})
    per_it = (flt["huber_1e6"]["ms"] / max(1, flt["huber_1e6"]["iter_sum"])) / (flt["plain"]["ms"] / max(1, flt["plain"]["iter_sum"]))
    print(json.dumps({"tool": "bench_ba_tracks_loss", "M": M, "windows": len(raw["tracks"]), "reps": REPS, "max_px": MAX_PX, "max_tracks": MAX_TRACKS, "scale": SCALE,
                      "raw": raw, "filtered": flt, "per_iteration_ratio": per_it}))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(arg("--worker", 4))
        sys.exit(0)
    lines = []
    for M in (4, 5, 6):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(M), "--reps", str(REPS), "--max-tracks", str(MAX_TRACKS), "--max-px", str(MAX_PX),
               "--scale", str(SCALE)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print("M = %d did not finish in %d s: stopping" % (M, LIMIT)); sys.exit(124)
        if r.returncode != 0:
            print("M = %d failed with status %d: stopping" % (M, r.returncode)); sys.exit(1)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        lines.append(json.loads(line))
    print(json.dumps({"tool": "bench_ba_tracks_loss", "summary": [
        {"M": l["M"], **{"raw_" + k: [round(l["raw"][k]["rot_deg_median"], 4), round(l["raw"][k]["t_deg_median"], 4), l["raw"][k]["iter_max"], round(l["raw"][k]["ms"], 3)]
                         for k in ("plain", "huber", "cauchy")},
         "filtered_ms": [round(l["filtered"]["plain"]["ms"], 3), round(l["filtered"]["huber_1e6"]["ms"], 3)], "per_iteration_ratio": round(l["per_iteration_ratio"], 3)}
        for l in lines]}))
