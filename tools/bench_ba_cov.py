"""What the covariance of the bundle adjustment costs on the polish of a dataset's triplet lists: the workload of tools/bench_ba_ragged.py -- every
triplet of the fountain and Herz-Jesu lists (tests/golden/epfl_all.npz), starts from pose_batch_ragged LinearTFT, triplets it refuses left out --, both
lists in ONE ragged call.  Three ways, alternated in one process, each timed over regions of --calls calls that end in a synchronise (host clock),
median of --reps regions after a warm-up, reported per call:
  (a) adjust          Context.bundle_adjust_ragged(...)                              -- what the parent commit did
  (b) adjust_cov      Context.bundle_adjust_ragged(..., cov=True)                     -- the adjustment followed by the covariance, one call
  (c) cov_alone       Context.ba_covariance_ragged(...) on the outputs of (a)
and (d), (e): (b) and (c) with point_cov=True.  The added cost (b) - (a) is also given as a share of (a).
Prints one JSON line.  usage: python tools/bench_ba_cov.py [--reps 9] [--calls 10] [--loss cauchy --scale 4]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from tft_vs_fund_amd import api


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS, CALLS = arg("--reps", 9), arg("--calls", 10)
LOSS, SCALE = arg("--loss", None, str), arg("--scale", None, float)
d = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "epfl_all.npz"))
ctx = api.Context(0)

items, calms, r2s, r3s = [], [], [], []
for name in ("fountain", "herzjesu"):
    off, K, trip = d[name + "_offsets"], d[name + "_K"], d[name + "_triplets"]
    S = off.shape[0] - 1
    cal = np.stack([np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0) for t in range(S)])
    lin = ctx.pose_batch_ragged("LinearTFTPoseEstimation", torch.from_numpy(np.ascontiguousarray(d[name + "_corresp"])).cuda(), torch.from_numpy(off).cuda(),
                                torch.from_numpy(cal).cuda(), reconst=False, n_max=int(np.diff(off).max()))
    ok = np.nonzero(lin["status"].cpu().numpy() == 0)[0]
    items += [d[name + "_corresp"][off[t]:off[t + 1]] for t in ok]
    calms.append(cal[ok]); r2s.append(lin["R_t_2"].cpu().numpy()[ok]); r3s.append(lin["R_t_3"].cpu().numpy()[ok])
pk, o2 = api.pack_ragged(items)
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
pk_d, off_d, calm_d, r2, r3 = cu(pk), cu(o2), cu(np.concatenate(calms)), cu(np.concatenate(r2s)), cu(np.concatenate(r3s))
kw = dict(loss=LOSS, scale=SCALE)

base = ctx.bundle_adjust_ragged(calm_d, r2, r3, pk_d, off_d, **kw)
p2, p3, rec = base["R_t_2"].contiguous(), base["R_t_3"].contiguous(), base["Reconst"]
ways = {
    "adjust": lambda: ctx.bundle_adjust_ragged(calm_d, r2, r3, pk_d, off_d, **kw),
    "adjust_cov": lambda: ctx.bundle_adjust_ragged(calm_d, r2, r3, pk_d, off_d, cov=True, **kw),
    "cov_alone": lambda: ctx.ba_covariance_ragged(calm_d, p2, p3, pk_d, off_d, rec, **kw),
    "adjust_cov_points": lambda: ctx.bundle_adjust_ragged(calm_d, r2, r3, pk_d, off_d, cov=True, point_cov=True, **kw),
    "cov_alone_points": lambda: ctx.ba_covariance_ragged(calm_d, p2, p3, pk_d, off_d, rec, point_cov=True, **kw),
}


def region(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / CALLS


full = ways["adjust_cov"]()
alone = ways["cov_alone"]()
torch.cuda.synchronize()
bits = lambda t: t.contiguous().view(torch.int64)
same = all(torch.equal(bits(full[k]), bits(base[k])) for k in ("R_t_2", "R_t_3", "repr_err")) and torch.equal(full["iter"], base["iter"])
composed = torch.equal(bits(full["cov"]), bits(alone["cov"])) and torch.equal(bits(full["sigma0"]), bits(alone["sigma0"]))
for fn in ways.values():                                                      # warm-up of every way
    fn()
times = {k: [] for k in ways}
for _ in range(REPS):
    for k, fn in ways.items():
        times[k].append(region(fn))
med = {k: float(np.median(v)) for k, v in times.items()}
n = np.diff(o2)
st = base["status"].cpu().numpy()
print(json.dumps({"tool": "bench_ba_cov", "reps": REPS, "calls_per_region": CALLS, "loss": LOSS, "scale": SCALE, "triplets": int(n.size), "matches": int(n.sum()),
                  "n_min": int(n.min()), "n_max": int(n.max()), "bad_status": int((st != 0).sum()), "iter_median": float(np.median(base["iter"].cpu().numpy())),
                  "nan_cov": int(torch.isnan(full["sigma0"]).sum().item()), "adjust_same_bits": bool(same), "cov_is_cov_alone": bool(composed),
                  "ms_per_call": {k: {"median": med[k], "min": float(np.min(v)), "max": float(np.max(v))} for k, v in times.items()},
                  "added_ms": med["adjust_cov"] - med["adjust"], "added_share_of_adjust": (med["adjust_cov"] - med["adjust"]) / med["adjust"]}))
