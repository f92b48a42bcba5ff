"""
Quality-guided (PROSAC) sampling in the robust estimators (tff_robust_pose_scenes_guided_*, tff_sample_indices_guided_dev; include/tftfund_guided.h).

The sampler is pinned bit for bit against its numpy twin (api.sample_indices_guided_reference), and the calls keep every bitwise contract of the uniform
ones: a scene of a list equals the one-scene call on it alone with seed + s, whatever the chunk or the round; the returned hypothesis is the earliest
arg-max of the counts rebuilt from the public pieces; with a confidence, used[s] is the existing stop rule on those counts.  quality= is order=; refine,
polish and the MSAC score compose as without a ranking.  The eight-scene run of a (method, score) is computed once and shared.
"""
import ctypes
import functools

import numpy as np
import pytest

import guided_cases as gc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

METHODS = ("LinearTFTPoseEstimation", "LinearFPoseEstimation")
KW = dict(candidates=4, lo_rounds=2)
N_HYP, FIRST, CONF, THR, SEED, GROWTH = 2049, 64, 0.99, 4.0, 20240, 1500
NAMES = ("inliers", "hypothesis", "refits", "candidates")
M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def _ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    return api.Context(0)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _bits(a):
    return np.ascontiguousarray(_np(a), dtype=np.float64).view(np.int64)


def _same(a, b):
    a, b = _np(a), _np(b)
    return np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _eight():
    """the eight scenes, their CalMs, and a shuffled ranking per scene, packed"""
    items, calms = gc.eight()
    rng = np.random.default_rng(77)
    orders = [rng.permutation(a.shape[0]).astype(np.int32) for a in items]
    return items, calms, orders


def _scenes_dev(method, items, calms, orders, n_hyp, seed, **more):
    from tft_vs_fund_amd import api
    packed, off = api.pack_ragged(items)
    out = _ctx().robust_pose_scenes(method, _cu(packed), _cu(off), _cu(calms), n_hyp, THR, seed=seed, ns_max=max(a.shape[0] for a in items),
                                    order=_cu(np.concatenate(orders)), growth=GROWTH, **{**KW, **more})
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}, packed, off


def _one_scene(method, scene, calm, order, n_hyp, seed, **more):
    out = _ctx().robust_pose(method, _cu(scene), _cu(calm), int(n_hyp), THR, seed=seed & M64, order=_cu(order), growth=GROWTH, **{**KW, **more})
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _assert_scene(out, off, s, ref, what):
    o0, o1 = int(off[s]), int(off[s + 1])
    assert int(out["status"][s]) == int(ref["status"]), (what, s, int(out["status"][s]), int(ref["status"]))
    assert [int(out[k][s]) for k in NAMES] == [int(ref[k]) for k in NAMES], (what, s)
    assert np.array_equal(out["mask"][o0:o1], ref["mask"]), (what, s)
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(out[k][s]), _bits(ref[k])), (what, s, k)


def _rebuilt_counts(method, scene, calm, order, seed, n_hyp, growth=GROWTH):
    """the counts of the hypotheses [0, n_hyp) from the public pieces; a failed hypothesis (a row of -1 included) counts -1"""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    d_scene, d_calm = _cu(scene), _cu(calm)
    idx = ctx.sample_indices_guided(seed & M64, 0, n_hyp, api.ROBUST_METHODS[method], _cu(order), growth)
    hyp = ctx.pose_sampled(method, d_scene, d_calm, idx)
    cnt = _np(ctx.inlier_count(d_scene, d_calm, hyp["R_t_2"], hyp["R_t_3"], THR)).astype(np.int64)
    cnt[_np(hyp["status"]) != 0] = -1
    return cnt, _np(idx)


# ---- 1. the sampler against its twin -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, (1 << 32) - 3])
@pytest.mark.parametrize("Ns, n, growth", [(7, 7, 1), (61, 7, 200000), (400, 8, 64)])
def test_sample_indices_guided_is_the_twin(Ns, n, growth, first):
    from tft_vs_fund_amd import api
    order = np.random.default_rng(Ns).permutation(Ns).astype(np.int32)
    got = _np(_ctx().sample_indices_guided(991, first, 1000, n, _cu(order), growth))
    assert got.dtype == np.int32 and np.array_equal(got, api.sample_indices_guided_reference(991, first, 1000, n, order, growth))


def test_growth_one_is_the_top_m_then_the_uniform_sampler():
    """growth = 1: hypothesis 0 draws the m best-ranked; the table still widens the pool by one per hypothesis (every step is ceil(...) >= 1), so the draw
    is the uniform sampler's through order from hypothesis ends[Ns] = Ns - m + 1 on -- from hypothesis 1 on when the scene is a single sample"""
    from tft_vs_fund_amd import api
    for Ns in (400, 7):
        order = np.random.default_rng(4).permutation(Ns).astype(np.int32)
        ends = api.guided_pool_ends(Ns, 7, 1)
        assert ends[Ns] == Ns - 7 + 1
        got = _np(_ctx().sample_indices_guided(5, 0, 500, 7, _cu(order), 1))
        uni = _np(_ctx().sample_indices(5, 0, 500, 7, Ns))
        assert sorted(got[0].tolist()) == sorted(order[:7].tolist()) and got[0, -1] == order[6]
        assert np.array_equal(got[ends[Ns]:], order[uni[ends[Ns]:]])
        if Ns > 7:
            assert not np.array_equal(got[:ends[Ns]], order[uni[:ends[Ns]]])


# ---- 2. the scenes contract --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shared(method, score):
    ctx = _ctx()
    items, calms, orders = _eight()
    ctx.set_score(score)
    try:
        out, packed, off = _scenes_dev(method, items, calms, orders, 300, SEED)
        refs = [_one_scene(method, items[s], calms[s], orders[s], 300, SEED + s) for s in range(len(items))]
    finally:
        ctx.set_score("count")
    return out, off, refs


def _check_contract(method, score):
    from tft_vs_fund_amd import api
    out, off, refs = _shared(method, score)
    assert "n_hyp_used" not in out and "n_hyp_used" not in refs[0]
    assert int(out["status"][6]) == api.ST_TOO_FEW and np.isnan(out["R_t_2"][6]).all()
    assert (out["status"][[0, 1, 2, 3, 7]] == 0).all()
    for s, ref in enumerate(refs):
        assert ref["R_t_2"].shape == (3, 4) and ref["T"].shape == (3, 3, 3)
        _assert_scene(out, off, s, ref, "%s %s" % (method, score))


@pytest.mark.parametrize("method", METHODS)
def test_every_scene_equals_its_one_scene_call(method):
    _check_contract(method, "count")


def test_every_scene_equals_its_one_scene_call_under_msac():
    _check_contract(METHODS[0], "msac")
    out, _, refs = _shared(METHODS[0], "msac")
    assert "score" in out and out["score"][6] == -1 and int(out["score"][1]) == int(refs[1]["score"])


# ---- 3. rebuilt from the public pieces -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_hypothesis_is_the_earliest_argmax_of_the_rebuilt_counts(method):
    items, calms, orders = _eight()
    s = 2                                                                     # 400 matches, 35 % outliers
    cnt, _ = _rebuilt_counts(method, items[s], calms[s], orders[s], SEED, 300)
    out = _one_scene(method, items[s], calms[s], orders[s], 300, SEED, lo_rounds=0)
    assert cnt.max() > 0 and int(out["status"]) == 0
    assert int(out["hypothesis"]) == int(np.argmax(cnt)) and int(out["inliers"]) == int(cnt.max())


# ---- 4. with a confidence ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_adaptive_is_the_fixed_guided_call_at_used_and_used_is_the_rule(method):
    from tft_vs_fund_amd import api
    items, calms, orders = _eight()
    out, _, off = _scenes_dev(method, items, calms, orders, N_HYP, SEED, confidence=CONF, first_round=FIRST)
    used = out["n_hyp_used"]
    assert used.dtype == np.int32 and used.shape == (8,) and used[6] == 0
    ends, qmin = api.round_plan(CONF, N_HYP, FIRST)
    n = api.ROBUST_METHODS[method]
    print("used:", used.tolist())
    for s in range(8):
        if s == 6:
            continue
        _assert_scene(out, off, s, _one_scene(method, items[s], calms[s], orders[s], used[s], SEED + s), "adaptive")
        cnt, _ = _rebuilt_counts(method, items[s], calms[s], orders[s], SEED + s, N_HYP)
        want = next((int(e) for e, q in zip(ends, qmin) if api.adaptive_stop(int(cnt[:e].max()), items[s].shape[0], n, q)), N_HYP)
        assert int(used[s]) == want, (s, int(used[s]), want)
    # robust_pose with a ranking and a confidence is the S = 1 call: n_hyp_used joins the dict
    one = _one_scene(method, items[1], calms[1], orders[1], N_HYP, SEED + 1, confidence=CONF, first_round=FIRST)
    assert int(one["n_hyp_used"]) == int(used[1])
    _assert_scene(out, off, 1, one, "robust_pose(confidence=, order=)")


# ---- 5. a chunk that cuts a scene ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hyp", [65536, 65536 + 1000])
def test_a_chunk_that_cuts_a_scene(n_hyp):
    """five scenes of 65 536 hypotheses exceed a chunk, which ends where scene 4 begins; with 66 536 every cut falls inside a scene"""
    from tft_vs_fund_amd import api
    method = METHODS[0]
    rng = np.random.default_rng(9)
    items = [np.ascontiguousarray(rng.uniform(0, 1000, (200, 6))) for _ in range(5)]
    orders = [rng.permutation(200).astype(np.int32) for _ in range(5)]
    calm = _eight()[1][0]
    assert 5 * n_hyp > api.ROBUST_CHUNK
    out, _, off = _scenes_dev(method, items, calm, orders, n_hyp, 77)
    for s in range(5):
        _assert_scene(out, off, s, _one_scene(method, items[s], calm, orders[s], n_hyp, 77 + s), "chunks")


# ---- 6. quality= is order= -----------------------------------------------------------------------------------------------------------------------------------
def test_quality_is_the_order_numpy_builds_from_it():
    from tft_vs_fund_amd import api
    ctx = _ctx()
    method = METHODS[0]
    items, calms, _ = _eight()
    items, calms = items[1:4], calms[1:4]
    packed, off = api.pack_ragged(items)
    rng = np.random.default_rng(21)
    quality = np.round(rng.normal(0, 1, packed.shape[0]), 1)                  # one decimal: many ties
    quality[off[1] + 17] = np.nan
    assert np.unique(quality[~np.isnan(quality)]).size < 100
    order = api.order_from_quality(quality, off)
    assert order[off[2] - 1] == 17                                            # NaN ranks last in its scene
    kw = dict(seed=SEED, growth=GROWTH, **KW)
    h_order = ctx.robust_pose_scenes(method, packed, off, calms, 300, THR, order=order, **kw)
    h_quality = ctx.robust_pose_scenes(method, packed, off, calms, 300, THR, quality=quality, **kw)
    dev = dict(ns_max=400, **kw)
    d_order = ctx.robust_pose_scenes(method, _cu(packed), _cu(off), _cu(calms), 300, THR, order=_cu(order), **dev)
    d_quality = ctx.robust_pose_scenes(method, _cu(packed), _cu(off), _cu(calms), 300, THR, quality=_cu(quality), **dev)
    d_quality32 = ctx.robust_pose_scenes(method, _cu(packed), _cu(off), _cu(calms), 300, THR, quality=_cu(quality.astype(np.float32)), **dev)
    torch.cuda.synchronize()
    assert (h_order["status"] == 0).all()
    for k in h_order:
        for other in (h_quality, d_order, d_quality, d_quality32):
            assert _same(h_order[k], other[k]), k
    # offsets[0] > 0 and entries behind offsets[S]: the packed entries outside the scenes, whatever their quality, take no part in a scene's ranking
    for front, back in ((-50.0, 50.0), (50.0, np.nan), (np.nan, -50.0)):
        packed2 = np.ascontiguousarray(np.concatenate([rng.uniform(0, 1000, (5, 6)), packed, rng.uniform(0, 1000, (3, 6))]))
        off2 = off + 5
        quality2 = np.concatenate([np.full(5, front), quality, np.full(3, back)])
        order2 = api.order_from_quality(quality2, off2)
        assert np.array_equal(order2[5:-3], order) and (order2[:5] == -1).all() and (order2[-3:] == -1).all()
        runs = [ctx.robust_pose_scenes(method, packed2, off2, calms, 300, THR, quality=quality2, **kw),
                ctx.robust_pose_scenes(method, _cu(packed2), _cu(off2), _cu(calms), 300, THR, quality=_cu(quality2), **dev),
                ctx.robust_pose_scenes(method, _cu(packed2), _cu(off2), _cu(calms), 300, THR, order=_cu(order2), **dev)]
        torch.cuda.synchronize()
        for other in runs:
            for k in h_order:
                want = np.concatenate([np.zeros(5, np.uint8), _np(h_order[k]), np.zeros(3, np.uint8)]) if k == "mask" else h_order[k]
                assert _same(want, other[k]), (front, back, k)
    uniform = ctx.robust_pose_scenes(method, packed, off, calms, 300, THR, seed=SEED, **KW)
    assert not _same(uniform["hypothesis"], h_order["hypothesis"])            # (the ranking is used at all)


# ---- 7. composition ------------------------------------------------------------------------------------------------------------------------------------------
def test_refine_and_polish_on_a_guided_result():
    from tft_vs_fund_amd import api
    ctx = _ctx()
    method = METHODS[0]
    items, calms, orders = _eight()
    pick = [0, 1, 2, 6, 7]
    items, calms, orders = [items[i] for i in pick], calms[pick], [orders[i] for i in pick]
    plain, packed, off = _scenes_dev(method, items, calms, orders, 300, SEED)
    out, _, _ = _scenes_dev(method, items, calms, orders, 300, SEED, refine="OptimFPoseEstimation", polish=True)
    for k, a in plain.items():
        assert _same(a, out[k]), k
    keep = plain["mask"] != 0
    cum = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
    r = ctx.pose_batch_ragged("OptimFPoseEstimation", _cu(packed[keep]), _cu(cum[off]), _cu(calms), reconst=False)
    ba = ctx.bundle_adjust_ragged(_cu(calms), _cu(plain["R_t_2"]), _cu(plain["R_t_3"]), _cu(packed), _cu(off), mask=_cu(plain["mask"]), reconst=False)
    torch.cuda.synchronize()
    for k, v in (("R_t_2_refined", r["R_t_2"]), ("R_t_3_refined", r["R_t_3"]), ("T_refined", r["T"]), ("iter_refined", r["iter"]),
                 ("status_refined", r["status"]), ("R_t_2_polished", ba["R_t_2"]), ("R_t_3_polished", ba["R_t_3"]), ("repr_err_polished", ba["repr_err"]),
                 ("iter_polished", ba["iter"]), ("status_polished", ba["status"])):
        assert _same(out[k], v), k
    assert out["status_refined"][0] == 0 and out["status_refined"][3] == api.ST_TOO_FEW
    # the one-scene call composes the same way, on the host path too
    one = ctx.robust_pose(method, items[1], calms[1], 300, THR, seed=SEED + 1, order=orders[1], growth=GROWTH, polish=True, **KW)
    assert isinstance(one["status"], int) and one["status"] == 0 and "n_hyp_used" not in one
    assert _same(one["R_t_2"], plain["R_t_2"][1]) and _same(one["R_t_2_polished"], out["R_t_2_polished"][1])


def test_growth_one_is_not_the_uniform_call():
    """one hypothesis: the guided call draws the seven best-ranked matches (true inliers here), the uniform call its own sample"""
    ctx = _ctx()
    scene, calm, inlier, quality = gc.use_case()
    order = np.argsort(-quality, kind="stable").astype(np.int32)
    assert inlier[order[:7]].all()
    g = ctx.robust_pose(METHODS[0], scene, calm, 1, THR, seed=3, order=order, growth=1, lo_rounds=0)
    u = ctx.robust_pose(METHODS[0], scene, calm, 1, THR, seed=3, lo_rounds=0)
    assert g["status"] == 0 and g["hypothesis"] == 0
    assert not _same(g["T"], u["T"])


# ---- 8. it does what it is for -----------------------------------------------------------------------------------------------------------------------------
def test_guided_sampling_finds_the_pose_the_uniform_budget_misses():
    """400 matches, 65 % outliers, 64 hypotheses: by the twins (tests/test_guided_cpu.py) the uniform sampler draws no all-inlier sample, the guided one
    all 64.  The guided call reaches at least 90 % of the inliers of LinearTFT on the true inliers alone (measured 2026-10-19: 140 of 140; the uniform
    call: 0).  The seeds were fixed by the twins before the first run (guided_cases.py).  The case is not typical: over the generator seeds 61 .. 72 and
    the call seeds 1, 2 the guided call at 64 hypotheses reaches the bound in 6 of 24 cases (4 of 24 with a noisier quality, sigma 0.5) and in 14 of 24 at
    256 hypotheses, the uniform call in none -- the early pools share most of their points and the seven-point solver is noise-sensitive, so even 64
    all-inlier samples are often not enough at this budget."""
    ctx = _ctx()
    method = METHODS[0]
    scene, calm, inlier, quality = gc.use_case()
    best = ctx.pose_batch(method, _cu(scene[inlier][None]), _cu(calm), reconst=False)
    bound = int(_np(ctx.inlier_count(_cu(scene), _cu(calm), best["R_t_2"], best["R_t_3"], THR))[0])
    out = ctx.robust_pose(method, scene, calm, gc.USE_N_HYP, THR, seed=gc.USE_CALL_SEED, quality=quality, growth=gc.USE_GROWTH)
    uni = ctx.robust_pose(method, scene, calm, gc.USE_N_HYP, THR, seed=gc.USE_CALL_SEED)
    print("inliers: true-inlier fit %d, guided %d (status %d), uniform %d (status %d)" % (bound, out["inliers"], out["status"], uni["inliers"], uni["status"]))
    assert out["status"] == 0 and out["inliers"] >= 0.9 * bound


# ---- 9. refusals on a live context ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_an_order_entry_out_of_range():
    from tft_vs_fund_amd import api
    ctx = _ctx()
    method = METHODS[0]
    items, calms, orders = _eight()
    scene, calm, order = items[2], calms[2], orders[2]
    d_scene, d_off, d_calm, d_order = _cu(scene), _cu(np.array([0, 400], dtype=np.int64)), _cu(calm.T.reshape(27)), _cu(order)
    outs = [torch.empty(n, dtype=t, device="cuda") for n, t in ((12, torch.float64), (12, torch.float64), (27, torch.float64), (400, torch.uint8),
                                                                (4, torch.int32), (1, torch.int32))]
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(order_t, growth, conf=0.0):
        Rt2, Rt3, T, mask, info, st = outs
        return ctx.lib.tff_robust_pose_scenes_guided_dev(ctx.handle, 0, p(d_scene), p(d_off), 400, 400, 1, p(d_calm), 0, 5, 100, 0, THR, 4, 1, conf, 64,
                                                         p(order_t), growth, p(Rt2), p(Rt3), p(T), p(mask), p(info), None, p(st))
    assert call(None, 100) == -10001 and b"null order" in ctx.lib.tff_last_error()
    for growth in (0, -1, api.GUIDED_MAX_GROWTH + 1):
        assert call(d_order, growth) == -10001 and b"growth" in ctx.lib.tff_last_error()
    assert call(d_order, 100, conf=0.99) == -10001                            # with a confidence `used` must be given
    assert call(d_order, 100, conf=1.5) == -10001
    assert call(d_order, 100) == 0                                            # a fixed n_hyp: `used` may be null
    d_used = torch.full((1,), -7, dtype=torch.int32, device="cuda")           # ... and if given it is filled with n_hyp
    Rt2, Rt3, T, mask, info, st = outs
    assert ctx.lib.tff_robust_pose_scenes_guided_dev(ctx.handle, 0, p(d_scene), p(d_off), 400, 400, 1, p(d_calm), 0, 5, 100, 0, THR, 4, 1, 0.0, 64,
                                                     p(d_order), 100, p(Rt2), p(Rt3), p(T), p(mask), p(info), p(d_used), p(st)) == 0
    torch.cuda.synchronize()
    assert d_used.cpu().tolist() == [100]
    h_used = np.full(1, -7, dtype=np.int32)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    h_out = [np.zeros(12), np.zeros(12), np.zeros(27), np.zeros(400, np.uint8), np.zeros(4, np.int32), np.zeros(1, np.int32)]
    h_off, h_calm = np.array([0, 400], dtype=np.int64), np.ascontiguousarray(calm.T).reshape(27)
    assert ctx.lib.tff_robust_pose_scenes_guided_host(ctx.handle, 0, hp(scene), hp(h_off), 1, hp(h_calm), 0, 5, 100, 0, THR, 4, 1, 0.0, 64, hp(order), 100,
                                                      *[hp(a) for a in h_out[:5]], hp(h_used), hp(h_out[5])) == 0
    assert h_used.tolist() == [100] and np.array_equal(h_out[4], info.cpu().numpy()) and np.array_equal(_bits(h_out[2]), _bits(T))
    assert ctx.lib.tff_sample_indices_guided_dev(ctx.handle, 1, 0, 10, 7, 400, None, 100, p(outs[4])) == -10001
    assert ctx.lib.tff_sample_indices_guided_dev(ctx.handle, 1, 0, 10, 7, 400, p(d_order), 0, p(outs[4])) == -10001
    assert ctx.lib.tff_sample_indices_guided_dev(ctx.handle, 1, 0, 10, 17, 400, p(d_order), 100, p(outs[4])) == -10001
    torch.cuda.synchronize()
    # entries out of range: no fault; the hypotheses that draw them are rows of -1 and count -1
    bad = order.copy()
    bad[[3, 50, 200]] = [-1, 400, 1 << 30]
    cnt, idx = _rebuilt_counts(method, scene, calm, bad, SEED, 300)
    ref_idx = api.sample_indices_guided_reference(SEED, 0, 300, 7, bad, GROWTH)
    assert np.array_equal(idx, ref_idx)
    dead = (idx == -1).all(axis=1)
    assert 0 < dead.sum() < 300 and (cnt[dead] == -1).all() and idx[~dead].min() >= 0
    out = _one_scene(method, scene, calm, bad, 300, SEED, lo_rounds=0)
    assert int(out["status"]) == 0 and int(out["hypothesis"]) == int(np.argmax(cnt)) and int(out["inliers"]) == int(cnt.max())
    assert not dead[int(out["hypothesis"])]
