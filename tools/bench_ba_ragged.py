"""The polish of a dataset's triplet list: BundleAdjustment on every triplet of the fountain and Herz-Jesu lists (tests/golden/epfl_all.npz, 150 triplets of
1 .. 1 400 matches and 56 of 70 .. 1 482), starts from pose_batch_ragged LinearTFT (triplets it refuses are left out).  Four ways, alternated in one
process, median of 7 after a warm-up, host clock around a synchronise:
  (a) ragged         ONE Context.bundle_adjust_ragged call under the default plan (TFF_OPT_BA_CLASSES = 0: one launch up to 256 items, three classes beyond);
  (b) grouped        a loop of fixed-N Context.bundle_adjust calls, one per distinct N -- what a user did before the ragged call existed;
  (c) one_class      the ragged call with all three class bounds set to TFF_BA_MAX_N (TFF_OPT_BA_CLASSES = 1): one launch sized for the largest item;
  (d) three_classes  the ragged call with three launch classes by LDS need (TFF_OPT_BA_CLASSES = 2).
Prints one JSON line.  usage: python tools/bench_ba_ragged.py [--reps 7]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from tft_vs_fund_amd import api

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
d = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "epfl_all.npz"))
ctx = api.Context(0)
result = {"tool": "bench_ba_ragged", "reps": REPS, "class_bounds": list(api.ba_ragged_class_bounds())}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for name in ("fountain", "herzjesu"):
    off, K, trip = d[name + "_offsets"], d[name + "_K"], d[name + "_triplets"]
    S = off.shape[0] - 1
    calms = np.stack([np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0) for t in range(S)])
    packed = torch.from_numpy(np.ascontiguousarray(d[name + "_corresp"])).cuda()
    lin = ctx.pose_batch_ragged("LinearTFTPoseEstimation", packed, torch.from_numpy(off).cuda(), torch.from_numpy(calms).cuda(), reconst=True,
                                n_max=int(np.diff(off).max()))
    ok = np.nonzero(lin["status"].cpu().numpy() == 0)[0]
    # the list without the refused triplets, packed again
    items = [d[name + "_corresp"][off[t]:off[t + 1]] for t in ok]
    pk, o2 = api.pack_ragged(items)
    pk_d, off_d = torch.from_numpy(pk).cuda(), torch.from_numpy(o2).cuda()
    calm_d = torch.from_numpy(calms[ok]).cuda()
    r2 = lin["R_t_2"][torch.from_numpy(ok).cuda()].contiguous(); r3 = lin["R_t_3"][torch.from_numpy(ok).cuda()].contiguous()
    n = np.diff(o2)
    groups = []                                                               # (b): one fixed-N batch per distinct N, gathered beforehand
    for N in sorted(set(n.tolist())):
        idx = np.nonzero(n == N)[0]
        C = torch.from_numpy(np.stack([items[i] for i in idx])).cuda()
        gi = torch.from_numpy(idx).cuda()
        groups.append((calm_d[gi].contiguous(), r2[gi].contiguous(), r3[gi].contiguous(), C))

    def ragged():
        return ctx.bundle_adjust_ragged(calm_d, r2, r3, pk_d, off_d)

    def grouped():
        return [ctx.bundle_adjust(*g) for g in groups]

    def with_plan(mode):
        ctx.set_ba_classes(mode)
        try:
            return ctx.bundle_adjust_ragged(calm_d, r2, r3, pk_d, off_d)
        finally:
            ctx.set_ba_classes(0)

    def one_class():
        return with_plan(1)

    def three_classes():
        return with_plan(2)

    a, c = three_classes(), one_class()
    torch.cuda.synchronize()
    same = all(torch.equal(a[k].view(torch.int64) if a[k].dtype == torch.float64 else a[k], c[k].view(torch.int64) if c[k].dtype == torch.float64 else c[k])
               for k in ("R_t_2", "R_t_3", "iter", "status"))
    grouped()                                                                 # warm-up of (b)
    three_classes(); ragged()                                                 # ... of the 80 and 160 KiB launches, and of the default plan
    times = {"ragged": [], "grouped": [], "one_class": [], "three_classes": []}
    for _ in range(REPS):
        times["ragged"].append(timed(ragged)); times["grouped"].append(timed(grouped)); times["one_class"].append(timed(one_class))
        times["three_classes"].append(timed(three_classes))
    cls = np.searchsorted(np.array(result["class_bounds"]), n)
    result[name] = {"triplets": int(ok.size), "distinct_n": len(groups), "n_min": int(n.min()), "n_max": int(n.max()),
                    "per_class": [int((cls == k).sum()) for k in range(3)], "bad_status": int((a["status"] != 0).sum()), "one_class_same_bits": bool(same),
                    "ms": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in times.items()}}
print(json.dumps(result))
