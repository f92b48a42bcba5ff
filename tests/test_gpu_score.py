"""
The MSAC score on the GPU (TFF_OPT_SCORE = 1, Context.set_score("msac")): include/tftfund.h states the weight of an inlier and what the robust estimators
do with the scores; these tests hold the library to that.

 1. every route of inlier_count / inlier_count_scenes gives the same int32 scores; count <= score <= 64 count with the hard counts of inlier_mask; the
    numpy bound of tests/test_emulated_score.py; the option set back to "count" reproduces the counts from before it was touched;
 2. robust_pose under MSAC equals, bit for bit, the algorithm rebuilt from the public pieces (as tests/test_gpu_robust.py::_definition, the scores in the
    places of the counts);
 3. robust_pose_scenes under MSAC: scene s = robust_pose alone with seed + s, host form = device form, a too-small scene keeps ST_TOO_FEW and score -1;
 4. the option's refusals; a fresh context counts.
Scenes: the config-4 recipe (0.5 px noise, a quarter of the matches displaced by U(20, 80) px in views 2 and 3).
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

METHODS = ("LinearTFTPoseEstimation", "LinearFPoseEstimation")
MASK64 = (1 << 64) - 1


def _ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    return api.Context(0)


@functools.lru_cache(maxsize=None)
def _synthetic(n, gen_seed):
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, n, noise=0.5, seed=gen_seed)
    scene = C[0].copy()
    rng = np.random.default_rng(gen_seed + 100)
    bad = rng.choice(n, n // 4, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    return np.ascontiguousarray(scene), np.ascontiguousarray(CalM)


def _config4_scene():
    """the scene of tests/test_gpu_robust.py: 400 matches, 100 displaced"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, 400, noise=0.5, seed=7)
    scene = C[0].copy()
    rng = np.random.default_rng(1)
    bad = rng.choice(400, 100, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    return np.ascontiguousarray(scene), np.ascontiguousarray(CalM)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _bits(a):
    return np.ascontiguousarray(_np(a), dtype=np.float64).view(np.int64)


def _poses(raw12):
    """(k, 12) column-major records -> (k, 3, 4)"""
    return raw12.reshape(-1, 4, 3).transpose(0, 2, 1)


# ---- 1. routes ------------------------------------------------------------------------------------------------------------------------------------------
ROUTE_SIZES = (16, 17, 65, 400, 1100)        # 1 100: above the 48 KB of the one-scene launcher (1 000) and the scenes kernel's staging bound (928)
N_HYP = 4099                                 # >= 4 096: the staged kernels; one tail hypothesis behind 256 full rows-wavefronts


def _numpy_count_and_F(ctx, scene, CalM, R2, R3, thr):
    """the rule and the untruncated weights in double on the points of the library's own triangulation: (count, F) per pose"""
    B, n = R2.shape[0], scene.shape[0]
    cams = np.zeros((B, 3, 3, 4))
    cams[:, 0] = CalM[0:3] @ np.eye(3, 4)
    cams[:, 1] = CalM[3:6] @ R2
    cams[:, 2] = CalM[6:9] @ R3
    X = ctx.triangulate(cams, np.ascontiguousarray(np.broadcast_to(scene, (B, n, 6))))
    torch.cuda.synchronize()
    X = X.cpu().numpy().transpose(0, 2, 1)                                    # (B, n, 4)
    c = 1.0 / (6.0 * thr * thr)
    cnt = np.zeros(B, dtype=np.int64); F = np.zeros(B)
    for b in range(B):
        ss = np.zeros(n); inl = np.ones(n, dtype=bool)
        for v in range(3):
            proj = X[b] @ cams[b, v].T
            with np.errstate(invalid="ignore", divide="ignore"):
                dx = proj[:, 0] / proj[:, 2] - scene[:, 2 * v]; dy = proj[:, 1] / proj[:, 2] - scene[:, 2 * v + 1]
                inl &= (np.abs(dx) <= thr) & (np.abs(dy) <= thr)
            ss += dx * dx + dy * dy
        cnt[b] = inl.sum()
        F[b] = (1.0 + 63.0 * (1.0 - ss[inl] * c)).sum()
    return cnt, F


@functools.lru_cache(maxsize=None)
def _route_hypotheses():
    """per scene size: (scene, CalM, R_t_2, R_t_3 (N_HYP, 3, 4) on the device) from LinearTFT on 7-point samples; computed once"""
    ctx = _ctx()
    out = []
    for k, n in enumerate(ROUTE_SIZES):
        scene, CalM = _synthetic(n, 20 + k)
        d_scene = torch.from_numpy(scene).cuda(); d_calm = torch.from_numpy(CalM).cuda()
        hyp = ctx.pose_sampled("LinearTFTPoseEstimation", d_scene, d_calm, ctx.sample_indices(31 + k, 0, N_HYP, 7, n))
        torch.cuda.synchronize()
        out.append((scene, CalM, hyp["R_t_2"].contiguous(), hyp["R_t_3"].contiguous()))
    return out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("k", range(len(ROUTE_SIZES)), ids=["Ns%d" % n for n in ROUTE_SIZES])
def test_every_route_gives_the_same_scores(k):
    from tft_vs_fund_amd import api
    scene, CalM, R2, R3 = _route_hypotheses()[k]
    ctx = _ctx()
    for thr in (4.0, 1.0):
        before = _np(ctx.inlier_count(scene, CalM, R2, R3, thr))
        ctx.set_score("msac")
        rows = _np(ctx.inlier_count(scene, CalM, R2, R3, thr))
        ctx.set_count_rows(0)
        staged = _np(ctx.inlier_count(scene, CalM, R2, R3, thr))
        ctx.set_count_rows(1)
        with_err, err = ctx.inlier_count(scene, CalM, R2, R3, thr, with_error=True)
        mask, hard = ctx.inlier_mask(scene, CalM, R2, R3, thr, with_counts=True)
        torch.cuda.synchronize()
        hard = _np(hard).astype(np.int64)
        assert np.array_equal(_np(mask).sum(axis=1, dtype=np.int64), hard) and _np(mask).max() <= 1     # the mask entry point stays hard
        assert np.array_equal(before, hard)
        assert np.array_equal(staged, rows) and np.array_equal(_np(with_err), rows), (thr, "count rows off / with_error")
        assert (hard <= rows).all() and (rows <= api.SCORE_UNITS * hard).all()
        top = np.argsort(-hard, kind="stable")[:5]                            # five hypotheses: the k_repr_error route
        t2 = R2[torch.from_numpy(top).cuda()]; t3 = R3[torch.from_numpy(top).cuda()]
        five = _np(ctx.inlier_count(scene, CalM, t2, t3, thr))
        assert np.array_equal(five, rows[top]), (thr, "five hypotheses")
        cnt, F = _numpy_count_and_F(ctx, scene, CalM, _np(t2), _np(t3), thr)
        print("Ns %d thr %g: best counts %s scores %s F %s" % (scene.shape[0], thr, hard[top].tolist(), five.tolist(), np.round(F, 1).tolist()))
        assert np.array_equal(cnt, hard[top])
        assert (F - cnt - 1 <= five).all() and (five <= F + 1).all()
        ctx.set_score("count")
        assert np.array_equal(_np(ctx.inlier_count(scene, CalM, R2, R3, thr)), before)


@pytest.mark.timeout(300)
def test_scenes_route_gives_the_same_scores():
    """the five scenes packed, 4 099 hypotheses each, against the one-scene scores and counts"""
    from tft_vs_fund_amd import api
    hyps = _route_hypotheses()
    ctx = _ctx()
    packed, off = api.pack_ragged([h[0] for h in hyps])
    calms = np.stack([h[1] for h in hyps])
    R2 = torch.cat([h[2] for h in hyps]); R3 = torch.cat([h[3] for h in hyps])
    for score in ("msac", "count"):
        ctx.set_score(score)
        got = _np(ctx.inlier_count_scenes(packed, off, calms, R2, R3, 4.0))
        ref = np.concatenate([_np(ctx.inlier_count(h[0], h[1], h[2], h[3], 4.0)) for h in hyps])
        assert np.array_equal(got, ref), score


# ---- 2. the estimator follows its definition ----------------------------------------------------------------------------------------------------------------
def _definition(ctx, method, scene, CalM, n_hyp, threshold, seed, candidates, lo_rounds):
    """Steps 1 - 4 of include/tftfund.h under TFF_OPT_SCORE = 1 from the public pieces: scores rank, adopt (>=) and pick; masks and inliers stay hard."""
    from tft_vs_fund_amd import api
    Ns = scene.shape[0]
    n = api.ROBUST_METHODS[method]
    d_scene = torch.from_numpy(scene).cuda(); d_calm = torch.from_numpy(CalM).cuda()
    idx = ctx.sample_indices(seed, 0, n_hyp, n, Ns)
    hyp = ctx.pose_sampled(method, d_scene, d_calm, idx)
    sco = ctx.inlier_count(d_scene, d_calm, hyp["R_t_2"], hyp["R_t_3"], threshold)
    torch.cuda.synchronize()
    st = hyp["status"].cpu().numpy(); sco = sco.cpu().numpy()
    ok = np.nonzero(st == 0)[0]
    order = ok[np.argsort(-sco[ok].astype(np.int64), kind="stable")][:candidates]
    assert order.size > 0
    sel = torch.from_numpy(order).cuda()
    r2, r3, tt = (t[sel].cpu().numpy() for t in hyp["_raw"])
    cur = sco[order].astype(np.int64)
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
    return dict(R_t_2=_poses(r2[w:w + 1])[0], R_t_3=_poses(r3[w:w + 1])[0], T=tt[w].reshape(3, 3, 3).transpose(2, 1, 0), mask=mask,
                hypothesis=int(order[w]), refits=int(nref[w]), candidates=int(order.size), score=int(cur[w]))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("threshold", (1.0, 4.0))
@pytest.mark.parametrize("method", METHODS)
def test_estimator_equals_its_definition_under_msac(method, threshold):
    ctx = _ctx()
    ctx.set_score("msac")
    scene, CalM = _config4_scene()
    out = ctx.robust_pose(method, torch.from_numpy(scene).cuda(), torch.from_numpy(CalM).cuda(), 2000, threshold, seed=1234, candidates=16, lo_rounds=2)
    assert out["score"].is_cuda
    torch.cuda.synchronize()
    ref = _definition(ctx, method, scene, CalM, 2000, threshold, 1234, 16, 2)
    print(method, threshold, "px: inliers %d score %d hypothesis %d refits %d" % (int(out["inliers"]), int(out["score"]), int(out["hypothesis"]), int(out["refits"])))
    assert int(out["status"]) == 0
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(out[k]), _bits(ref[k])), k
    mask = _np(out["mask"])
    assert np.array_equal(mask, ref["mask"])
    for k in ("hypothesis", "refits", "candidates", "score"):
        assert int(out[k]) == ref[k], (k, int(out[k]), ref[k])
    assert int(out["inliers"]) == int(mask.sum())


# ---- 3. scenes ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_scenes_under_msac_equal_the_one_scene_call(method):
    from tft_vs_fund_amd import api
    ctx = _ctx()
    ctx.set_score("msac")
    sizes = (5, api.ROBUST_METHODS[method], 9, 16, 61, 400, 1400)
    items = [_synthetic(n, 40 + k) for k, n in enumerate(sizes)]
    scenes = [a for a, _ in items]; calms = np.stack([c for _, c in items])
    packed, off = api.pack_ragged(scenes)
    seed = MASK64 - 2                                                         # the seed wraps at scene 3
    dev = ctx.robust_pose_scenes(method, torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(calms).cuda(), 1001, 4.0,
                                 seed=seed, ns_max=1400)
    assert dev["score"].is_cuda
    torch.cuda.synchronize()
    dev = {k: _np(v) for k, v in dev.items()}
    host = ctx.robust_pose_scenes(method, packed, off, calms, 1001, 4.0, seed=seed)
    keys = ("inliers", "hypothesis", "refits", "candidates", "status", "score", "mask")
    for k in keys:
        assert np.array_equal(np.asarray(host[k]), dev[k]), k
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(host[k]), _bits(dev[k])), k
    assert int(dev["status"][0]) == api.ST_TOO_FEW and int(dev["score"][0]) == -1 and int(dev["inliers"][0]) == 0
    for s in range(1, len(sizes)):
        one = ctx.robust_pose(method, torch.from_numpy(scenes[s]).cuda(), torch.from_numpy(calms[s]).cuda(), 1001, 4.0, seed=(seed + s) & MASK64)
        torch.cuda.synchronize()
        assert int(one["status"]) == int(dev["status"][s]) == 0, s
        for k in ("inliers", "hypothesis", "refits", "candidates", "score"):
            assert int(one[k]) == int(dev[k][s]), (s, k, int(one[k]), int(dev[k][s]))
        assert np.array_equal(_np(one["mask"]), dev["mask"][off[s]:off[s + 1]]), s
        assert int(dev["inliers"][s]) == int(dev["mask"][off[s]:off[s + 1]].sum()), s
        for k in ("R_t_2", "R_t_3", "T"):
            assert np.array_equal(_bits(one[k]), _bits(dev[k][s])), (s, k)
    print(method, "inliers", dev["inliers"].tolist(), "scores", dev["score"].tolist())


# ---- 4. arguments ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_option_refusals_and_the_default():
    from tft_vs_fund_amd import api
    ctx = _ctx()
    scene, CalM = _config4_scene()
    d_scene = torch.from_numpy(scene).cuda(); d_calm = torch.from_numpy(CalM).cuda()
    hyp = ctx.pose_sampled("LinearTFTPoseEstimation", d_scene, d_calm, ctx.sample_indices(5, 0, 64, 7, 400))
    fresh = _np(ctx.inlier_count(d_scene, d_calm, hyp["R_t_2"], hyp["R_t_3"], 4.0))
    _, hard = ctx.inlier_mask(d_scene, d_calm, hyp["R_t_2"], hyp["R_t_3"], 4.0, with_counts=True)
    assert np.array_equal(fresh, _np(hard))                                   # a fresh context counts
    assert "score" not in ctx.robust_pose("LinearTFTPoseEstimation", d_scene, d_calm, 500, 4.0, seed=1)
    set_option = ctx.lib.tff_ctx_set_option
    for bad in (2, -1):
        assert set_option(ctx.handle, api.TFF_OPT_SCORE, ctypes.c_long(bad)) == -10001
    assert np.array_equal(_np(ctx.inlier_count(d_scene, d_calm, hyp["R_t_2"], hyp["R_t_3"], 4.0)), fresh)   # a refused value changes nothing
    assert set_option(ctx.handle, api.TFF_OPT_SCORE, ctypes.c_long(1)) == 0
    msac = _np(ctx.inlier_count(d_scene, d_calm, hyp["R_t_2"], hyp["R_t_3"], 4.0))
    assert (msac >= fresh).all() and not np.array_equal(msac, fresh)
    with pytest.raises(ValueError):
        ctx.set_score("nonsense")
