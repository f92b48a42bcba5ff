"""
Robust pose estimation for a batch of scenes in one call (tff_robust_pose_scenes_*, tff_inlier_count_scenes_dev).

The contract is bitwise (include/tftfund.h): scene s of a call gets what the EXISTING one-scene call -- Context.robust_pose, Context.inlier_count -- gives
for that scene alone with seed + s.  Every comparison here is against that call: poses and T as bit patterns, mask, info and status exactly.  The
one-scene results are computed once per (method, arguments) and shared.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

METHODS = ("LinearTFTPoseEstimation", "LinearFPoseEstimation")
MASK64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def _ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    return api.Context(0)


@functools.lru_cache(maxsize=None)
def _synthetic(n, gen_seed):
    """the config-4 recipe of tests/test_gpu_robust.py at n correspondences: 0.5 px noise, a quarter of the matches displaced by U(20, 80) px in views 2, 3"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, n, noise=0.5, seed=gen_seed)
    scene = C[0].copy()
    rng = np.random.default_rng(gen_seed + 100)
    bad = rng.choice(n, n // 4, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    return np.ascontiguousarray(scene), np.ascontiguousarray(CalM)


@functools.lru_cache(maxsize=None)
def _epfl():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epfl_all.npz"))
    return {k: d[k] for k in ("fountain_offsets", "fountain_corresp", "fountain_K", "fountain_triplets")}


def _fountain(t):
    d = _epfl()
    off, K, trip = d["fountain_offsets"], d["fountain_K"], d["fountain_triplets"]
    return np.ascontiguousarray(d["fountain_corresp"][off[t]:off[t + 1]]), np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0)


def _large_fountain():
    """the first fountain triplet with more than 1 000 correspondences: above the LDS staging bound of the count kernel (928), its own CalM"""
    t = int(np.nonzero(np.diff(_epfl()["fountain_offsets"]) > 1000)[0][0])
    return _fountain(t)


def _seven(method):
    """5 (too few), n_sample, 9, 16, 61, 400 synthetic correspondences and the large fountain triplet; a CalM per scene"""
    from tft_vs_fund_amd import api
    sizes = (5, api.ROBUST_METHODS[method], 9, 16, 61, 400)
    items = [_synthetic(n, 7 + k) for k, n in enumerate(sizes)] + [_large_fountain()]
    assert items[-1][0].shape[0] > 1000
    return [a for a, _ in items], np.stack([c for _, c in items])


def _bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _one_scene(method, scene, CalM, n_hyp, threshold, seed, kw):
    """the reference: the existing one-scene call.  A scene it refuses for its size (Ns < n_sample) is the batch call's ST_TOO_FEW."""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    n = kw.get("n_sample") or api.ROBUST_METHODS[method]
    if scene.shape[0] < n:
        return None
    out = ctx.robust_pose(method, torch.from_numpy(scene).cuda(), torch.from_numpy(CalM).cuda(), n_hyp, threshold, seed=seed & MASK64, **kw)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _assert_scene(method, out, offsets, s, ref, what):
    """scene s of the batch result `out` (numpy) against the one-scene result, or against the contract of an invalid scene when ref is an int status"""
    o0, o1 = int(offsets[s]), int(offsets[s + 1])
    info = np.array([out[k][s] for k in ("inliers", "hypothesis", "refits", "candidates")])
    if isinstance(ref, int):
        assert int(out["status"][s]) == ref, (what, s, int(out["status"][s]))
        assert info.tolist() == [0, -1, 0, 0], (what, s, info)
        for k in ("R_t_2", "R_t_3", "T"):
            assert np.isnan(out[k][s]).all(), (what, s, k)
        if ref == 1:                                                          # ST_TOO_FEW: the range is the scene's own (bad offsets name no range)
            assert not out["mask"][o0:o1].any(), (what, s)
        return
    assert int(out["status"][s]) == int(ref["status"]), (what, s, int(out["status"][s]), int(ref["status"]))
    rinfo = np.array([int(ref[k]) for k in ("inliers", "hypothesis", "refits", "candidates")])
    assert np.array_equal(info, rinfo), (what, s, info, rinfo)
    assert np.array_equal(out["mask"][o0:o1], ref["mask"]), (what, s)
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(out[k][s]), _bits(ref[k])), (what, s, k)


def _run_dev(method, items, calm, n_hyp, threshold, seed, offsets=None, ns_max=None, **kw):
    from tft_vs_fund_amd import api
    ctx = _ctx()
    packed, off = api.pack_ragged(items)
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.int64)
    if ns_max is None:
        ns_max = max(a.shape[0] for a in items)
    out = ctx.robust_pose_scenes(method, torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(calm)).cuda(),
                                 n_hyp, threshold, seed=seed, ns_max=ns_max, **kw)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}, off


def _compare_all(method, items, calms, n_hyp, threshold, seed, what, **kw):
    from tft_vs_fund_amd import api
    out, off = _run_dev(method, items, calms, n_hyp, threshold, seed, **kw)
    for s, scene in enumerate(items):
        ref = _one_scene(method, scene, calms[s] if calms.ndim == 3 else calms, n_hyp, threshold, seed + s, kw)
        _assert_scene(method, out, off, s, api.ST_TOO_FEW if ref is None else ref, what)
    return out, off


# ---- 1. every scene equals its one-scene call ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_every_scene_equals_its_one_scene_call(method):
    from tft_vs_fund_amd import api
    items, calms = _seven(method)
    for rounds in (0, 2):                                                     # 1001 hypotheses per scene: wavefronts and count slabs straddle scenes
        out, _ = _compare_all(method, items, calms, 1001, 4.0, 1234, (method, "lo_rounds", rounds), candidates=4, lo_rounds=rounds)
        assert int(out["status"][0]) == api.ST_TOO_FEW and (out["status"][1:] != api.ST_BAD_OFFSETS).all()
        print(method, "lo_rounds", rounds, "inliers", out["inliers"].tolist(), "status", out["status"].tolist())
    _compare_all(method, items, calms, 3, 4.0, 1234, (method, "n_hyp 3"), candidates=4, lo_rounds=2)   # fewer hypotheses than rows or candidates
    _compare_all(method, items, calms, 1001, 4.0, 1234, (method, "n_sample 10"), candidates=4, lo_rounds=2, n_sample=10)   # (the 9-match scene: too few)


# ---- 2. across a chunk boundary -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_across_a_chunk_boundary(method):
    from tft_vs_fund_amd import api
    n_hyp = 100000
    assert 2 * n_hyp < api.ROBUST_CHUNK < 3 * n_hyp                            # the boundary cuts the third scene
    items = [_synthetic(61, 40 + k)[0] for k in range(3)]
    calms = np.stack([_synthetic(61, 40 + k)[1] for k in range(3)])
    _compare_all(method, items, calms, n_hyp, 4.0, 1234, (method, "chunks"), candidates=4, lo_rounds=2)


# ---- 3. the real list -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("method", METHODS)
def test_the_fountain_list(method):
    from tft_vs_fund_amd import api
    d = _epfl()
    off = d["fountain_offsets"]
    S = off.shape[0] - 1
    assert S == 150 and int(np.diff(off).min()) == 1
    pairs = [_fountain(t) for t in range(S)]
    items = [a for a, _ in pairs]
    calms = np.stack([c for _, c in pairs])
    out, _ = _compare_all(method, items, calms, 500, 4.0, 77, (method, "fountain"), candidates=4, lo_rounds=2)
    few = np.diff(off) < api.ROBUST_METHODS[method]
    assert np.array_equal(out["status"] == api.ST_TOO_FEW, few) and few.any()
    print(method, "fountain: %d triplets, %d too few, %d without a pose, median inlier share %.3f"
          % (S, int(few.sum()), int((out["status"] == api.ST_NO_POSE).sum()), float(np.median(out["inliers"][~few] / np.diff(off)[~few]))))


# ---- 4. bad offsets on the device -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_bad_offsets_on_the_device(method):
    """scenes 0 and 3 are valid; scene 1 has a decreasing offset, scene 2 more correspondences than ns_max allows"""
    from tft_vs_fund_amd import api
    a, calm = _synthetic(61, 11)
    b = _synthetic(40, 12)[0]
    big = _synthetic(400, 13)[0][:100]
    packed = [a, big, b]                                                      # 61 + 100 + 40 correspondences
    offsets = [0, 61, 40, 161, 201]                                           # scene 1: 61 -> 40 decreases; scene 2 = [40, 161): 121 > ns_max
    out, off = _run_dev(method, packed, calm, 300, 4.0, 5, offsets=offsets, ns_max=61, candidates=4, lo_rounds=2)
    kw = dict(candidates=4, lo_rounds=2)
    _assert_scene(method, out, off, 0, _one_scene(method, a, calm, 300, 4.0, 5, kw), "valid 0")
    _assert_scene(method, out, off, 1, api.ST_BAD_OFFSETS, "decreasing")
    _assert_scene(method, out, off, 2, api.ST_BAD_OFFSETS, "n_s > ns_max")
    _assert_scene(method, out, off, 3, _one_scene(method, b, calm, 300, 4.0, 8, kw), "valid 3")
    assert not out["mask"][61:161].any()                                      # nothing was written outside the valid scenes' ranges
    # an offset above n_total
    out, off = _run_dev(method, [a], calm, 300, 4.0, 5, offsets=[0, 61, 70], ns_max=61, candidates=4, lo_rounds=2)
    _assert_scene(method, out, off, 0, _one_scene(method, a, calm, 300, 4.0, 5, kw), "valid before")
    _assert_scene(method, out, off, 1, api.ST_BAD_OFFSETS, "above n_total")


# ---- 5. the _host form, determinism, the seed -------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_host_form_determinism_and_seed_wrap(method):
    from tft_vs_fund_amd import api
    ctx = _ctx()
    items = [_synthetic(n, 20 + k)[0] for k, n in enumerate((61, 5, 400, 16))]
    calm = _synthetic(61, 20)[1]
    seed = (1 << 64) - 2                                                      # scenes 2 and 3 draw with the seeds 0 and 1
    kw = dict(candidates=4, lo_rounds=2)
    dev, off = _compare_all(method, items, calm, 700, 4.0, seed, (method, "wrap"), **kw)
    again, _ = _run_dev(method, items, calm, 700, 4.0, seed, **kw)
    packed, offsets = api.pack_ragged(items)
    host = ctx.robust_pose_scenes(method, packed, offsets, calm, 700, 4.0, seed=seed, **kw)
    for other, what in ((again, "same seed twice"), (host, "_host")):
        for k in ("status", "inliers", "hypothesis", "refits", "candidates", "mask"):
            assert np.array_equal(np.asarray(other[k]), dev[k]), (what, k)
        for k in ("R_t_2", "R_t_3", "T"):
            assert np.array_equal(_bits(other[k]), _bits(dev[k])), (what, k)
    assert isinstance(host["mask"], np.ndarray) and host["R_t_2"].shape == (4, 3, 4) and host["T"].shape == (4, 3, 3, 3)
    with pytest.raises(ValueError):
        ctx.robust_pose_scenes(method, packed, np.array([0, 70, 61, 482, 498]), calm, 700, 4.0)   # _host: bad offsets are refused


# ---- 6. inlier_count_scenes ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _count_inputs():
    """four scenes (9, 61, 400 synthetic, 1 400 real correspondences), 5 000 poses each: minimal-sample hypotheses of the scene itself, a few set to NaN"""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    d = _epfl()
    t = int(np.nonzero(np.diff(d["fountain_offsets"]) == 1400)[0][0])
    pairs = [_synthetic(9, 31), _synthetic(61, 32), _synthetic(400, 33), _fountain(t)]
    assert [a.shape[0] for a, _ in pairs] == [9, 61, 400, 1400]
    poses = []
    for k, (scene, calm) in enumerate(pairs):
        idx = ctx.sample_indices(50 + k, 0, 5000, 7, scene.shape[0])
        hyp = ctx.pose_sampled("LinearTFTPoseEstimation", torch.from_numpy(scene).cuda(), torch.from_numpy(calm).cuda(), idx)
        r2, r3 = hyp["R_t_2"].contiguous(), hyp["R_t_3"].contiguous()
        r2[[3, 4000]] = float("nan")
        poses.append((r2, r3))
    torch.cuda.synchronize()
    return pairs, poses


@pytest.mark.timeout(300)
@pytest.mark.parametrize("per_scene", (1, 3, 4, 1001, 5000))
def test_inlier_count_scenes(per_scene):
    """5 000 >= 4 096: the one-scene reference takes its row kernel (staged in LDS; the 1 400-match scene k_repr_error); below, k_repr_error"""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    pairs, poses = _count_inputs()
    packed, offsets = api.pack_ragged([a for a, _ in pairs])
    calms = np.stack([c for _, c in pairs])
    r2 = torch.cat([p[0][:per_scene] for p in poses]); r3 = torch.cat([p[1][:per_scene] for p in poses])
    d_packed = torch.from_numpy(packed).cuda(); d_off = torch.from_numpy(offsets).cuda()
    for thr in (1.0, 4.0):
        got = ctx.inlier_count_scenes(d_packed, d_off, calms, r2, r3, thr)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for s, (scene, calm) in enumerate(pairs):
            ref = ctx.inlier_count(scene, calm, poses[s][0][:per_scene], poses[s][1][:per_scene], thr)
            torch.cuda.synchronize()
            assert np.array_equal(got[s * per_scene:(s + 1) * per_scene], ref.cpu().numpy()), (per_scene, thr, s)
        print("per_scene %d, %g px: best counts %s" % (per_scene, thr, [int(got[s * per_scene:(s + 1) * per_scene].max()) for s in range(4)]))
    # a scene with bad offsets counts -1, its neighbours as before
    bad = offsets.copy(); bad[2] = bad[1] - 1                                 # scene 1 decreases; scene 2 = [bad[2], offsets[3]) is another scene but valid
    got_bad = ctx.inlier_count_scenes(d_packed, torch.from_numpy(bad).cuda(), calms, r2, r3, 4.0).cpu().numpy()
    assert (got_bad[per_scene:2 * per_scene] == -1).all()
    assert np.array_equal(got_bad[:per_scene], got[:per_scene]) and np.array_equal(got_bad[3 * per_scene:], got[3 * per_scene:])


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_refusals():
    from tft_vs_fund_amd import api
    ctx = _ctx()
    dev = torch.device("cuda", 0)
    scene, CalM = _synthetic(61, 11)
    packed, offsets = api.pack_ragged([scene, scene[:40]])
    d_sc = torch.from_numpy(packed).cuda(); d_off = torch.from_numpy(offsets).cuda()
    d_calm = torch.from_numpy(np.ascontiguousarray(CalM.T).reshape(27)).cuda()
    canary = 7
    outs = dict(Rt2=torch.empty((2, 12), dtype=torch.float64, device=dev), Rt3=torch.empty((2, 12), dtype=torch.float64, device=dev),
                T=torch.empty((2, 27), dtype=torch.float64, device=dev), mask=torch.empty(101, dtype=torch.uint8, device=dev),
                info=torch.empty((2, 4), dtype=torch.int32, device=dev), status=torch.empty(2, dtype=torch.int32, device=dev))
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(**kw):
        a = dict(method=0, scenes=d_sc, offsets=d_off, n_total=101, ns_max=61, S=2, calm=d_calm, calm_stride=0, seed=1, n_hyp=100, n_sample=0,
                 threshold=4.0, n_cand=4, lo_rounds=1, **outs)
        a.update(kw)
        return ctx.lib.tff_robust_pose_scenes_dev(ctx.handle, a["method"], p(a["scenes"]), p(a["offsets"]), a["n_total"], a["ns_max"], a["S"], p(a["calm"]),
                                                  a["calm_stride"], a["seed"], a["n_hyp"], a["n_sample"], a["threshold"], a["n_cand"], a["lo_rounds"],
                                                  p(a["Rt2"]), p(a["Rt3"]), p(a["T"]), p(a["mask"]), p(a["info"]), p(a["status"]))
    assert call() == 0
    torch.cuda.synchronize()
    assert outs["status"].cpu().tolist() == [0, 0]
    bad = [dict(method=1), dict(method=7), dict(method=-1), dict(n_sample=6), dict(method=6, n_sample=7), dict(n_sample=17), dict(n_hyp=0), dict(n_hyp=-5),
           dict(n_cand=0), dict(n_cand=65), dict(lo_rounds=-1), dict(lo_rounds=9), dict(threshold=0.0), dict(threshold=float("nan")),
           dict(threshold=float("inf")), dict(scenes=None), dict(calm=None), dict(offsets=None),
           dict(S=-1), dict(S=3, n_hyp=(1 << 31) // 3 + 1), dict(S=1 << 22, n_cand=64), dict(calm_stride=9), dict(calm_stride=-27),
           dict(n_total=-1), dict(n_total=1 << 31), dict(ns_max=-1), dict(ns_max=(1 << 24) + 1)] + [{k: None} for k in outs]
    for t in outs.values():                                                   # a refused call launches nothing: the outputs keep the canary
        t.fill_(canary)
    torch.cuda.synchronize()
    for kw in bad:
        assert call(**kw) == -10001, kw
    ctx.set_rows(0)                                                           # as the ragged call refuses it
    assert call() == -10001
    ctx.set_rows("auto")
    ctx.set_kernel_variant(1)
    assert call() == -10001
    ctx.set_kernel_variant(0)
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == canary).all()), k
    assert call(S=0) == 0
    torch.cuda.synchronize()
    assert bool((outs["status"] == canary).all())
    # the _host form shares the checks, and refuses offsets the device form turns into statuses
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    h = dict(Rt2=np.empty((2, 12)), Rt3=np.empty((2, 12)), T=np.empty((2, 27)), mask=np.zeros(101, dtype=np.uint8), info=np.zeros((2, 4), dtype=np.int32),
             status=np.zeros(2, dtype=np.int32))
    calm_h = np.ascontiguousarray(CalM.T).reshape(27)

    def host(off, S=2, n_cand=4):
        off = np.asarray(off, dtype=np.int64)
        return ctx.lib.tff_robust_pose_scenes_host(ctx.handle, 0, hp(packed), hp(off), S, hp(calm_h), 0, 1, 100, 0, 4.0, n_cand, 1, hp(h["Rt2"]), hp(h["Rt3"]),
                                                   hp(h["T"]), hp(h["mask"]), hp(h["info"]), hp(h["status"]))
    assert host([0, 61, 101]) == 0 and h["status"].tolist() == [0, 0]
    assert host([0, 61, 40]) == -10001 and host([-1, 61, 101]) == -10001 and host([0, 61, 101], n_cand=0) == -10001
    assert host([0, 61, 101], S=0) == 0
    # the count call
    r = torch.zeros((2, 12), dtype=torch.float64, device=dev); cnt = torch.full((2,), canary, dtype=torch.int32, device=dev)

    def count(**kw):
        a = dict(scenes=d_sc, offsets=d_off, n_total=101, S=2, calm=d_calm, calm_stride=0, Rt2=r, Rt3=r, per_scene=1, threshold=4.0, counts=cnt)
        a.update(kw)
        return ctx.lib.tff_inlier_count_scenes_dev(ctx.handle, p(a["scenes"]), p(a["offsets"]), a["n_total"], a["S"], p(a["calm"]), a["calm_stride"],
                                                   p(a["Rt2"]), p(a["Rt3"]), a["per_scene"], a["threshold"], p(a["counts"]))
    for kw in (dict(S=-1), dict(per_scene=-1), dict(n_total=-1), dict(n_total=1 << 31), dict(calm_stride=5), dict(S=1 << 20, per_scene=1 << 20),
               dict(scenes=None), dict(offsets=None), dict(calm=None), dict(Rt2=None), dict(Rt3=None), dict(counts=None)):
        assert count(**kw) == -10001, kw
    assert count(S=0) == 0 and count(per_scene=0) == 0
    torch.cuda.synchronize()
    assert bool((cnt == canary).all())
    with pytest.raises(ValueError):
        ctx.robust_pose_scenes("ResslTFTPoseEstimation", d_sc, d_off, CalM, 100, 4.0)
