"""
Robust three-view pose estimation on the GPU (tff_sample_indices_dev, tff_inlier_mask_batch_dev, tff_robust_pose_*).

The estimator's contract is bitwise: include/tftfund.h fixes the algorithm in terms of the library's public pieces, and `_definition` below rebuilds
it from them -- Context.sample_indices, pose_sampled, inlier_count, a stable sort, inlier_mask, numpy compaction, pose_batch_ragged, inlier_count -- and
the result is compared as bit patterns.  The scene is that of tools/config4_ransac.py: 400 correspondences at 0.5 px noise, 100 of them displaced by
U(20, 80) px in views 2 and 3.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

METHODS = ("LinearTFTPoseEstimation", "LinearFPoseEstimation")
SHAPES = [(7, 400), (8, 9), (16, 16), (8, 8), (7, 1400)]


def _ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    return api.Context(0)


def _config4_scene():
    """(scene (400, 6), CalM, the two ground-truth poses, displaced (400,) bool)"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, Rt0, _ = generate_scene_batch(1, 400, noise=0.5, seed=7)
    scene = C[0].copy()
    rng = np.random.default_rng(1)
    bad = rng.choice(400, 100, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    displaced = np.zeros(400, dtype=bool)
    displaced[bad] = True
    return scene, CalM, Rt0, displaced


def _epfl_scene():
    """the first fountain triplet with more than 1 000 correspondences, and its CalM"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epfl_all.npz"))
    off, cor, K, trip = d["fountain_offsets"], d["fountain_corresp"], d["fountain_K"], d["fountain_triplets"]
    t = int(np.nonzero(np.diff(off) > 1000)[0][0])
    return np.ascontiguousarray(cor[off[t]:off[t + 1]]), np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0)


def _bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _poses(raw12):
    """(k, 12) column-major records -> (k, 3, 4)"""
    return raw12.reshape(-1, 4, 3).transpose(0, 2, 1)


def _definition(ctx, method, scene, CalM, n_hyp, threshold, seed=0, n_sample=None, candidates=16, lo_rounds=2):
    """Steps 1-4 of include/tftfund.h from the public pieces.  Returns dict(R_t_2, R_t_3, T, mask, info (4,), status, best_sampled)."""
    from tft_vs_fund_amd import api
    Ns = scene.shape[0]
    n = n_sample or api.ROBUST_METHODS[method]
    d_scene = torch.from_numpy(scene).cuda(); d_calm = torch.from_numpy(CalM).cuda()
    idx = ctx.sample_indices(seed, 0, n_hyp, n, Ns)
    hyp = ctx.pose_sampled(method, d_scene, d_calm, idx)
    cnt = ctx.inlier_count(d_scene, d_calm, hyp["R_t_2"], hyp["R_t_3"], threshold)
    torch.cuda.synchronize()
    st = hyp["status"].cpu().numpy(); cnt = cnt.cpu().numpy()
    ok = np.nonzero(st == 0)[0]
    order = ok[np.argsort(-cnt[ok].astype(np.int64), kind="stable")][:candidates]
    if order.size == 0:
        return dict(status=api.ST_NO_POSE, info=np.array([0, -1, 0, 0]), mask=np.zeros(Ns, dtype=np.uint8), best_sampled=0)
    sel = torch.from_numpy(order).cuda()
    r2, r3, tt = (t[sel].cpu().numpy() for t in hyp["_raw"])
    cur = cnt[order].astype(np.int64)
    nref = np.zeros(order.size, dtype=np.int64)
    for _ in range(lo_rounds):
        mask = ctx.inlier_mask(d_scene, d_calm, _poses(r2), _poses(r3), threshold).cpu().numpy()
        corresp, offsets = api.pack_ragged([scene[mask[r] != 0] for r in range(order.size)])
        ref = ctx.pose_batch_ragged(method, torch.from_numpy(corresp).cuda(), torch.from_numpy(offsets).cuda(), d_calm, reconst=False, n_max=Ns)
        rc = ctx.inlier_count(d_scene, d_calm, ref["R_t_2"], ref["R_t_3"], threshold).cpu().numpy()
        rst = ref["status"].cpu().numpy()
        f2, f3, ft = (t.cpu().numpy() for t in ref["_raw"][:3])
        adopt = (rst == 0) & (rc >= cur)
        r2[adopt], r3[adopt], tt[adopt] = f2[adopt], f3[adopt], ft[adopt]
        cur[adopt] = rc[adopt]
        nref += adopt
    w = int(np.argmax(cur))                                                   # the first of the largest
    mask = ctx.inlier_mask(d_scene, d_calm, _poses(r2[w:w + 1]), _poses(r3[w:w + 1]), threshold).cpu().numpy()[0]
    assert int(mask.sum()) == int(cur[w])
    return dict(R_t_2=_poses(r2[w:w + 1])[0], R_t_3=_poses(r3[w:w + 1])[0], T=tt[w].reshape(3, 3, 3).transpose(2, 1, 0), mask=mask,
                info=np.array([int(cur[w]), int(order[w]), int(nref[w]), int(order.size)]), status=0, best_sampled=int(cnt[ok].max()))


def _run(ctx, method, scene, CalM, n_hyp, threshold, **kw):
    out = ctx.robust_pose(method, torch.from_numpy(scene).cuda(), torch.from_numpy(CalM).cuda(), n_hyp, threshold, **kw)
    torch.cuda.synchronize()
    return out


def _info(out):
    return np.array([int(out[k]) for k in ("inliers", "hypothesis", "refits", "candidates")])


def _assert_equal(out, ref, what):
    assert int(out["status"]) == ref["status"], what
    assert np.array_equal(_info(out), ref["info"]), (what, _info(out), ref["info"])
    m = out["mask"].cpu().numpy() if hasattr(out["mask"], "cpu") else out["mask"]
    assert np.array_equal(m, ref["mask"]), what
    assert int(m.sum()) == int(out["inliers"]), what
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(out[k]), _bits(ref[k])), (what, k)


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_sampler_equals_its_definition():
    from tft_vs_fund_amd import api
    ctx = _ctx()
    for n, Ns in SHAPES:
        for seed, first in ((1234, 0), (2 ** 63 + 11, 0), (1234, (1 << 33) + 5)):
            got = ctx.sample_indices(seed, first, 3000, n, Ns)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), api.sample_indices_reference(seed, first, 3000, n, Ns)), (n, Ns, seed, first)
    assert ctx.sample_indices(1, 0, 0, 7, 400).shape == (0, 7)
    for bad in ((0, 0, 4, 0, 400), (0, 0, 4, 17, 400), (0, 0, 4, 8, 7), (0, -1, 4, 7, 400), (0, 0, -1, 7, 400)):
        with pytest.raises(api.TffError):
            ctx.sample_indices(*bad)


# ---- the inlier flags ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_mask_row_sums_equal_the_counts_on_every_route(method):
    from tft_vs_fund_amd import api
    ctx = _ctx()
    scene, CalM, _, _ = _config4_scene()
    d_scene = torch.from_numpy(scene).cuda(); d_calm = torch.from_numpy(CalM).cuda()
    idx = ctx.sample_indices(77, 0, 8192, api.ROBUST_METHODS[method], 400)
    hyp = ctx.pose_sampled(method, d_scene, d_calm, idx)
    for t in hyp["_raw"]:
        t[[5, 50, 5000]] = float("nan")                                       # what a failed hypothesis leaves in every output
    torch.cuda.synchronize()
    print("failed hypotheses among 8192:", int((hyp["status"] != 0).sum()), "+ 3 set to NaN")
    for thr in (1.0, 4.0):
        mask, mcnt = ctx.inlier_mask(d_scene, d_calm, hyp["R_t_2"], hyp["R_t_3"], thr, with_counts=True)
        torch.cuda.synchronize()
        mask = mask.cpu().numpy(); sums = mask.sum(axis=1, dtype=np.int64)
        assert mask.max() <= 1
        assert np.array_equal(mcnt.cpu().numpy(), sums)
        for B, rows in ((100, 1), (8192, 1), (8192, 0)):                       # k_repr_error, k_inlier_count_rows, k_inlier_count_staged
            ctx.set_count_rows(rows)
            cnt = ctx.inlier_count(d_scene, d_calm, hyp["R_t_2"][:B], hyp["R_t_3"][:B], thr)
            torch.cuda.synchronize()
            assert np.array_equal(cnt.cpu().numpy(), sums[:B]), (thr, B, rows)
        ctx.set_count_rows(1)
        print("threshold %g: best count %d" % (thr, int(sums.max())))


@pytest.mark.timeout(300)
def test_mask_of_the_true_poses_is_the_undisplaced_set():
    """At 4 px the ground-truth cameras accept exactly the 300 undisplaced correspondences (the numpy oracle: at least 16 px of margin on the displaced
    entries, 8 sigma on the others, so rounding cannot move an entry)."""
    ctx = _ctx()
    scene, CalM, Rt0, displaced = _config4_scene()
    mask, cnt = ctx.inlier_mask(scene, CalM, Rt0[0][None], Rt0[1][None], 4.0, with_counts=True)
    torch.cuda.synchronize()
    assert np.array_equal(mask.cpu().numpy()[0] != 0, ~displaced)
    assert int(cnt[0]) == 300


# ---- the estimator equals its definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("method", METHODS)
def test_estimator_equals_its_definition_small(method):
    ctx = _ctx()
    scene, CalM, _, _ = _config4_scene()
    for rounds in (0, 1, 3):
        kw = dict(seed=1234, candidates=4, lo_rounds=rounds)
        _assert_equal(_run(ctx, method, scene, CalM, 1000, 4.0, **kw), _definition(ctx, method, scene, CalM, 1000, 4.0, **kw), (method, rounds))
    kw = dict(seed=3, n_sample=10)
    _assert_equal(_run(ctx, method, scene, CalM, 5000, 4.0, **kw), _definition(ctx, method, scene, CalM, 5000, 4.0, **kw), (method, "n_sample 10"))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("method", METHODS)
def test_estimator_equals_its_definition_across_chunks(method):
    from tft_vs_fund_amd import api
    ctx = _ctx()
    scene, CalM, _, _ = _config4_scene()
    n_hyp = max(300000, 2 * api.ROBUST_CHUNK + 1000)
    out = _run(ctx, method, scene, CalM, n_hyp, 4.0, seed=1234)
    ref = _definition(ctx, method, scene, CalM, n_hyp, 4.0, seed=1234)
    print(method, n_hyp, "hypotheses:", _info(out).tolist())
    _assert_equal(out, ref, method)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("method", METHODS)
def test_estimator_equals_its_definition_on_a_large_real_triplet(method):
    ctx = _ctx()
    scene, CalM = _epfl_scene()
    assert scene.shape[0] > 1000
    for thr in (4.0, 1.0):
        out = _run(ctx, method, scene, CalM, 3000, thr, seed=5, candidates=8)
        ref = _definition(ctx, method, scene, CalM, 3000, thr, seed=5, candidates=8)
        print(method, "fountain triplet of", scene.shape[0], "at", thr, "px:", _info(out).tolist())
        _assert_equal(out, ref, (method, thr))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_host_form_determinism_and_seed(method):
    ctx = _ctx()
    scene, CalM, _, _ = _config4_scene()
    dev = _run(ctx, method, scene, CalM, 4000, 4.0, seed=9)
    again = _run(ctx, method, scene, CalM, 4000, 4.0, seed=9)
    host = ctx.robust_pose(method, scene, CalM, 4000, 4.0, seed=9)
    for other, what in ((again, "same seed twice"), (host, "_host")):
        assert int(other["status"]) == int(dev["status"]) == 0
        assert np.array_equal(_info(other), _info(dev)), what
        assert np.array_equal(np.asarray(other["mask"].cpu() if hasattr(other["mask"], "cpu") else other["mask"]), dev["mask"].cpu().numpy()), what
        for k in ("R_t_2", "R_t_3", "T"):
            assert np.array_equal(_bits(other[k]), _bits(dev[k])), (what, k)
    assert int(_run(ctx, method, scene, CalM, 4000, 4.0, seed=10)["hypothesis"]) != int(dev["hypothesis"])


# ---- it does what it is for -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_pose_from_matches_with_outliers(method):
    """Config-4 scene, 4 px, 20 000 hypotheses, seed 1234, K = 16, two rounds.  No displaced correspondence in the final mask; the final count not below
    the best sampled hypothesis's; pose errors below those of the plain fit to all 400 matches.  LinearTFT in addition: at least 98 % of the count
    that the existing pose_batch on the 300 undisplaced correspondences reaches (the numpy oracle reaches 300 of 300 from eleven of sixteen candidates;
    the 2 % is for fixpoints that differ by borderline correspondences).  LinearF: the count is printed, not bounded."""
    from tft_vs_fund_amd.metrics import AngError_batch
    ctx = _ctx()
    scene, CalM, Rt0, displaced = _config4_scene()
    out = _run(ctx, method, scene, CalM, 20000, 4.0, seed=1234)
    ref = _definition(ctx, method, scene, CalM, 20000, 4.0, seed=1234)

    def errors(R2, R3):
        r2, t2 = AngError_batch(Rt0[0], np.asarray(R2)[None]); r3, t3 = AngError_batch(Rt0[1], np.asarray(R3)[None])
        return 0.5 * float(r2[0] + r3[0]), 0.5 * float(t2[0] + t3[0])
    rot, tr = errors(out["R_t_2"].cpu().numpy(), out["R_t_3"].cpu().numpy())
    plain = ctx.pose_batch(method, scene[None], CalM, reconst=False)
    rot_all, tr_all = errors(plain["R_t_2"][0], plain["R_t_3"][0])
    clean = ctx.pose_batch(method, np.ascontiguousarray(scene[~displaced])[None], CalM, reconst=False)
    clean_cnt = int(ctx.inlier_count(scene, CalM, clean["R_t_2"], clean["R_t_3"], 4.0)[0])
    mask = out["mask"].cpu().numpy() != 0
    print("%s: inliers %d (best sampled %d, clean-set fit %d), hypothesis %d, refits %d, candidates %d; rot / t error %.4f / %.4f deg (all 400: %.3f / %.3f)"
          % (method, int(out["inliers"]), ref["best_sampled"], clean_cnt, int(out["hypothesis"]), int(out["refits"]), int(out["candidates"]), rot, tr,
             rot_all, tr_all))
    assert int(out["status"]) == 0
    assert not (mask & displaced).any()
    assert int(out["inliers"]) >= ref["best_sampled"]
    assert rot < rot_all and tr < tr_all
    if method == "LinearTFTPoseEstimation":
        assert int(out["inliers"]) >= 0.98 * clean_cnt


@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_nothing_succeeds(method):
    from tft_vs_fund_amd import api
    ctx = _ctx()
    scene, CalM, _, _ = _config4_scene()
    scene[:, 0] = np.nan                                                      # every correspondence carries a NaN: no sample can succeed
    d_scene = torch.from_numpy(scene).cuda(); d_calm = torch.from_numpy(CalM).cuda()
    hyp = ctx.pose_sampled(method, d_scene, d_calm, ctx.sample_indices(21, 0, 2000, api.ROBUST_METHODS[method], 400))
    torch.cuda.synchronize()
    assert int((hyp["status"] == 0).sum()) == 0
    for out in (_run(ctx, method, scene, CalM, 2000, 4.0, seed=21), ctx.robust_pose(method, scene, CalM, 2000, 4.0, seed=21)):
        assert int(out["status"]) == api.ST_NO_POSE
        assert int(out["inliers"]) == 0 and int(out["candidates"]) == 0
        for k in ("R_t_2", "R_t_3", "T"):
            assert np.isnan(np.asarray(out[k].cpu() if hasattr(out[k], "cpu") else out[k])).all(), k
        assert not np.asarray(out["mask"].cpu() if hasattr(out["mask"], "cpu") else out["mask"]).any()


# ---- refusals and the refinement convenience ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_refusals():
    from tft_vs_fund_amd import api
    ctx = _ctx()
    scene, CalM, _, _ = _config4_scene()
    dev = torch.device("cuda", 0)
    d_scene = torch.from_numpy(scene).cuda(); d_calm = torch.from_numpy(np.ascontiguousarray(CalM.T).reshape(27)).cuda()
    outs = dict(Rt2=torch.empty(12, dtype=torch.float64, device=dev), Rt3=torch.empty(12, dtype=torch.float64, device=dev),
                T=torch.empty(27, dtype=torch.float64, device=dev), mask=torch.empty(400, dtype=torch.uint8, device=dev),
                info=torch.empty(4, dtype=torch.int32, device=dev), status=torch.empty(1, dtype=torch.int32, device=dev))
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def call(fn="tff_robust_pose_dev", **kw):
        a = dict(method=0, scene=d_scene, Ns=400, calm=d_calm, seed=1, n_hyp=100, n_sample=0, threshold=4.0, n_cand=4, lo_rounds=1, **outs)
        a.update(kw)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        return getattr(ctx.lib, fn)(ctx.handle, a["method"], p(a["scene"]), a["Ns"], p(a["calm"]), a["seed"], a["n_hyp"], a["n_sample"], a["threshold"],
                                    a["n_cand"], a["lo_rounds"], p(a["Rt2"]), p(a["Rt3"]), p(a["T"]), p(a["mask"]), p(a["info"]), p(a["status"]))
    assert call() == 0
    torch.cuda.synchronize()
    bad = [dict(method=1), dict(method=7), dict(method=-1), dict(method=8), dict(n_sample=6), dict(method=6, n_sample=7), dict(n_sample=17),
           dict(Ns=6), dict(method=6, Ns=7), dict(n_sample=12, Ns=11), dict(n_hyp=0), dict(n_hyp=-5), dict(n_cand=0), dict(n_cand=65),
           dict(lo_rounds=-1), dict(lo_rounds=9), dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")),
           dict(scene=None), dict(calm=None)] + [{k: None} for k in outs]
    for kw in bad:
        assert call(**kw) == -10001, kw
    host = dict(scene=None)                                                  # (the _host form shares the checks: one probe)
    assert call("tff_robust_pose_host", **host) == -10001
    ctx.set_rows(0)
    assert call() == -10001
    ctx.set_rows("auto")
    ctx.set_kernel_variant(1)
    assert call() == -10001
    ctx.set_kernel_variant(0)
    assert call() == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ctx.robust_pose("ResslTFTPoseEstimation", scene, CalM, 100, 4.0)


@pytest.mark.timeout(300)
def test_refine_is_the_fixed_n_call_on_the_inliers():
    ctx = _ctx()
    scene, CalM, _, _ = _config4_scene()
    out = ctx.robust_pose("LinearTFTPoseEstimation", torch.from_numpy(scene).cuda(), torch.from_numpy(CalM).cuda(), 5000, 4.0, seed=2,
                          refine="ResslTFTPoseEstimation")
    torch.cuda.synchronize()
    mask = out["mask"].cpu().numpy() != 0
    ref = ctx.pose_batch("ResslTFTPoseEstimation", torch.from_numpy(np.ascontiguousarray(scene[mask])[None]).cuda(), torch.from_numpy(CalM).cuda(),
                         reconst=False)
    torch.cuda.synchronize()
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(out[k + "_refined"]), _bits(ref[k][0])), k
    assert int(out["iter_refined"]) == int(ref["iter"][0]) and int(out["status_refined"]) == int(ref["status"][0]) == 0
    host = ctx.robust_pose("LinearTFTPoseEstimation", scene, CalM, 5000, 4.0, seed=2, refine="ResslTFTPoseEstimation")
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(host[k + "_refined"]), _bits(ref[k][0])), k


# ---- the one-scene call is the scene-list chain at S = 1 ----------------------------------------------------------------------------------------------
def _small_scene(n, clean):
    """the config-4 recipe at n correspondences (a quarter displaced); clean: no noise and nothing displaced, so that a sample of all n has a pose"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, n, noise=0.0 if clean else 0.5, seed=11 + n)
    scene = C[0].copy()
    if not clean:
        rng = np.random.default_rng(n)
        bad = rng.choice(n, n // 4, replace=False)
        scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    return np.ascontiguousarray(scene), np.ascontiguousarray(CalM)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _assert_same_result(got, ref, what, keys=("mask", "inliers", "hypothesis", "refits", "candidates", "status")):
    """two result dicts of the same shapes: poses and T as bit patterns, everything else exactly"""
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (what, k)
    for k in keys + (("score",) if "score" in ref else ()):
        assert np.array_equal(_np(got[k]), _np(ref[k])), (what, k, _np(got[k]), _np(ref[k]))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_one_scene_call_equals_the_explicit_one_scene_list(method):
    """robust_pose (device tensors: no offsets reach the library; numpy: the offsets {0, Ns} are made by the library) against robust_pose_scenes with the
    explicit offsets [0, Ns] and the shared (9, 3) CalM, bit for bit.  Ns = one sample, 65 and 257; 5 hypotheses for 16 candidates (keys of 0 reach seed,
    offsets, compaction and finish), 1 000 hypotheses without and with refits; under both scores."""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    n = api.ROBUST_METHODS[method]
    try:
        for score in ("count", "msac"):
            ctx.set_score(score)
            for Ns in (n, 65, 257):
                scene, CalM = _small_scene(Ns, clean=Ns == n)
                d_scene = torch.from_numpy(scene).cuda(); d_calm = torch.from_numpy(CalM).cuda()
                d_off = torch.tensor([0, Ns], dtype=torch.int64).cuda()
                for n_hyp, cand, rounds in ((5, 16, 2), (1000, 16, 0), (1000, 16, 2)):
                    kw = dict(seed=77, candidates=cand, lo_rounds=rounds)
                    what = (method, score, Ns, n_hyp, rounds)
                    lst = ctx.robust_pose_scenes(method, d_scene, d_off, d_calm, n_hyp, 4.0, ns_max=Ns, **kw)
                    dev = ctx.robust_pose(method, d_scene, d_calm, n_hyp, 4.0, **kw)
                    torch.cuda.synchronize()
                    host = ctx.robust_pose(method, scene, CalM, n_hyp, 4.0, **kw)
                    assert lst["status"].shape == (1,) and lst["mask"].shape == (Ns,)
                    one = {k: (v if k == "mask" else v[0]) for k, v in lst.items()}
                    _assert_same_result(dev, one, what + ("device",))
                    _assert_same_result(host, one, what + ("host",))
                    if Ns == n:
                        assert int(dev["status"]) == 0 and int(dev["inliers"]) == Ns, what   # noise-free: the one sample there is has a pose
                    if n_hyp == 5:
                        assert int(dev["candidates"]) <= 5, what
    finally:
        ctx.set_score("count")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_shared_calm_equals_a_copy_per_scene(method):
    """S = 3 scenes of 40, 7 and 300 matches: the shared (9, 3) CalM (handed to the pose kernels as it is) gives bit for bit what (S, 9, 3) holding three
    copies of it gives (one copy per hypothesis row), on the device and the host path."""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    scenes = [_small_scene(40, False), _small_scene(7, True), _small_scene(300, False)]
    CalM = scenes[0][1]
    assert all(np.array_equal(c, CalM) for _, c in scenes)                    # (generate_scene_batch: one calibration)
    packed, off = api.pack_ragged([a for a, _ in scenes])
    copies = np.ascontiguousarray(np.stack([CalM] * 3))
    kw = dict(seed=5, candidates=8, lo_rounds=2)
    keys = ("mask", "inliers", "hypothesis", "refits", "candidates", "status")
    d = lambda a: torch.from_numpy(a).cuda()
    shared = ctx.robust_pose_scenes(method, d(packed), d(off), d(CalM), 500, 4.0, ns_max=300, **kw)
    per = ctx.robust_pose_scenes(method, d(packed), d(off), d(copies), 500, 4.0, ns_max=300, **kw)
    torch.cuda.synchronize()
    _assert_same_result(shared, per, (method, "device"), keys)
    assert _np(shared["status"])[[0, 2]].tolist() == [0, 0]
    assert int(_np(shared["status"])[1]) == (0 if api.ROBUST_METHODS[method] == 7 else api.ST_TOO_FEW)
    h_shared = ctx.robust_pose_scenes(method, packed, off, CalM, 500, 4.0, **kw)
    h_per = ctx.robust_pose_scenes(method, packed, off, copies, 500, 4.0, **kw)
    _assert_same_result(h_shared, h_per, (method, "host"), keys)
    _assert_same_result(h_shared, shared, (method, "host against device"), keys)
