"""Do partially visible tracks improve a window's poses?  And what does per-point visibility cost where it is not needed?

Windows of M = 4, 5, 6 consecutive views of fountain-P11 and Herz-Jesu-P8 (tests/golden/epfl_all.npz): the matches of consecutive triplets that agree to the
bit in the two views they share are merged into tracks, tracks whose reprojection under the ground-truth cameras exceeds 1 px in any seen coordinate are
removed (experiments_real.m:93-99 does that per triplet), at most --max-tracks tracks of a window are kept by a fixed seed (the points live in LDS).  Every
window starts from the ground-truth poses perturbed by a fixed seed (~0.5 degrees, 1 %).  Per M, all windows of both datasets:
  (a) tracks        Context.bundle_adjust_views(..., missing="point") over ALL tracks, one batch padded with NaN columns
  (b) full_view     Context.bundle_adjust_views(...) over the fully visible tracks only, one call per window (the whole-view call cannot be padded)
  (c) full_point    missing="point" over those same fully visible tracks, one call per window like (b); and (c_batch) the same as one padded batch
For each: the median rotation and translation error of the cameras 2 .. M of every window against the ground truth (metrics.AngError_batch, degrees) and
the time of the call(s), host clock around a synchronise, median of --reps after a warm-up.  cost_of_visibility = (c) / (b).
Each M runs in a child process under its own time limit (--limit seconds); the first child that fails or runs out of time ends the run.
Prints one JSON line per M, then one summary line.  usage: python tools/bench_ba_tracks.py [--reps 7] [--max-tracks 2000] [--limit 240]"""
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


REPS, MAX_TRACKS, LIMIT = arg("--reps", 7), arg("--max-tracks", 2000), arg("--limit", 240)
IMAGES = {"fountain": 11, "herzjesu": 8}


def windows(M):
    import ba_tracks_cases as tc
    out = []
    for ds, n_img in IMAGES.items():
        for first in range(1, n_img - M + 2):
            C, CalM, R_t, _ = tc.window_tracks(ds, first, M)
            rng = np.random.default_rng(1000 * M + first)
            if C.shape[1] > MAX_TRACKS:
                C = np.ascontiguousarray(C[:, np.sort(rng.permutation(C.shape[1])[:MAX_TRACKS])])
            out.append(dict(name="%s %d..%d" % (ds, first, first + M - 1), C=C, CalM=CalM, R_t=R_t, R0=tc._perturbed(R_t, rng)))
    return out


def worker(M):
    import torch
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.metrics import AngError_batch
    import ba_tracks_oracle as TO
    ws = windows(M)
    ctx = api.Context(0)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for w in ws:
        w["full"] = TO.visibility(w["C"]).all(axis=0)
        G = np.vstack([w["R_t"][0:3], [0, 0, 0, 1]])
        w["truth"] = [w["R_t"][3 * j:3 * j + 3] @ np.linalg.inv(G) for j in range(1, M)]         # cameras 2 .. M in the frame of camera 1

    def padded(key):
        n = max(int(w[key].sum()) if key else w["C"].shape[1] for w in ws)
        Cs = []
        for w in ws:
            C = w["C"][:, w[key]] if key else w["C"]
            Cs.append(np.hstack([C, np.full((2 * M, n - C.shape[1]), np.nan)]).T)
        return cu(np.stack([w["CalM"] for w in ws])), cu(np.stack([w["R0"] for w in ws])), cu(np.stack(Cs))

    all_in, full_in = padded(None), padded("full")
    per_window = [(cu(w["CalM"]), cu(w["R0"][None]), cu(w["C"][:, w["full"]].T[None])) for w in ws]
    ways = {
        "tracks": lambda: [ctx.bundle_adjust_views(*all_in, missing="point")],
        "full_view": lambda: [ctx.bundle_adjust_views(*a) for a in per_window],
        "full_point": lambda: [ctx.bundle_adjust_views(*a, missing="point") for a in per_window],
        "full_point_batch": lambda: [ctx.bundle_adjust_views(*full_in, missing="point")],
    }

    def errors(outs):
        R = torch.cat([o["R_t"] for o in outs]).cpu().numpy(); st = torch.cat([o["status"] for o in outs]).cpu().numpy()
        it = torch.cat([o["iter"] for o in outs]).cpu().numpy()
        rot, tr = [], []
        for b, w in enumerate(ws):
            for j in range(1, M):
                r, t = AngError_batch(w["truth"][j - 1], R[b:b + 1, 3 * j:3 * j + 3])
                rot.append(float(r[0])); tr.append(float(t[0]))
        return dict(rot_deg_median=float(np.median(rot)), t_deg_median=float(np.median(tr)), bad_status=int((st != 0).sum()), iter_median=float(np.median(it)))

    res = {}
    for k, fn in ways.items():                                                           # results and warm-up
        outs = fn(); torch.cuda.synchronize()
        res[k] = errors(outs)
    start_rot, start_t = [], []
    for w in ws:
        G = np.vstack([w["R0"][0:3], [0, 0, 0, 1]])
        for j in range(1, M):
            r, t = AngError_batch(w["truth"][j - 1], (w["R0"][3 * j:3 * j + 3] @ np.linalg.inv(G))[None])
            start_rot.append(float(r[0])); start_t.append(float(t[0]))
    times = {k: [] for k in ways}
    for _ in range(REPS):
        for k, fn in ways.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
    for k in ways:
        res[k].update(ms=float(np.median(times[k])), ms_min=float(np.min(times[k])), ms_max=float(np.max(times[k])), calls=len(ws) if k in ("full_view", "full_point") else 1)
    nv = np.concatenate([TO.visibility(w["C"]).sum(axis=0) for w in ws])
    print(json.dumps({"tool": "bench_ba_tracks", "M": M, "windows": len(ws), "reps": REPS, "tracks": [int(w["C"].shape[1]) for w in ws],
                      "fully_visible": [int(w["full"].sum()) for w in ws], "seen_in": {str(v): int((nv == v).sum()) for v in range(2, M + 1)},
                      "start": dict(rot_deg_median=float(np.median(start_rot)), t_deg_median=float(np.median(start_t))), **res,
                      "cost_of_visibility": res["full_point"]["ms"] / res["full_view"]["ms"]}))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(arg("--worker", 4))
        sys.exit(0)
    lines = []
    for M in (4, 5, 6):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(M), "--reps", str(REPS), "--max-tracks", str(MAX_TRACKS)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print("M = %d did not finish in %d s: stopping" % (M, LIMIT)); sys.exit(124)
        if r.returncode != 0:
            print("M = %d failed with status %d: stopping" % (M, r.returncode)); sys.exit(1)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        lines.append(json.loads(line))
    print(json.dumps({"tool": "bench_ba_tracks", "summary": [
        {"M": l["M"], **{k: [round(l[k]["rot_deg_median"], 4), round(l[k]["t_deg_median"], 4), round(l[k]["ms"], 3)] for k in ("tracks", "full_view", "full_point", "full_point_batch")},
         "cost_of_visibility": round(l["cost_of_visibility"], 3)} for l in lines]}))
