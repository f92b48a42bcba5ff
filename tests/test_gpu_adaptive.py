"""
Robust pose estimation with an early stop per scene (tff_robust_pose_scenes_adaptive_*: a confidence and a cap instead of a fixed number of hypotheses).

The contract is bitwise (include/tftfund.h): scene s gets what the EXISTING one-scene call, Context.robust_pose, gives for it alone with n_hyp = used[s]
and seed + s.  And used[s] itself is the stop rule applied to the counts of the scene's hypotheses: those are rebuilt here from the public pieces
(sample_indices, pose_sampled, inlier_count) and the rule is applied in numpy (api.adaptive_stop) with the thresholds of api.round_plan.
The eight-scene run of a (method, score) is computed once and shared by the tests that read it.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

METHODS = ("LinearTFTPoseEstimation", "LinearFPoseEstimation")
KW = dict(candidates=4, lo_rounds=2)
N_HYP, FIRST, CONF, THR, SEED = 2049, 64, 0.99, 4.0, 20240
OUTLIER_SHARES = (0.20, 0.35, 0.50, 0.65)
NAMES = ("inliers", "hypothesis", "refits", "candidates")


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


def _contaminated(n, share, gen_seed):
    """the recipe of tools/config4_ransac.py: 0.5 px noise, `share` of the matches displaced by U(20, 80) px in views 2 and 3"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, n, noise=0.5, seed=gen_seed)
    scene = C[0].copy()
    rng = np.random.default_rng(gen_seed + 100)
    bad = rng.choice(n, int(share * n), replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    return np.ascontiguousarray(scene), np.ascontiguousarray(CalM)


@functools.lru_cache(maxsize=None)
def _eight():
    """noise-free 200 | 400 with 20, 35, 50, 65 % outliers | 200 random matches | 5 matches | a fountain triplet with more than 300 matches; a CalM each"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, 200, noise=0.0, seed=31)
    items = [(np.ascontiguousarray(C[0]), np.ascontiguousarray(CalM))]
    items += [_contaminated(400, share, 41 + k) for k, share in enumerate(OUTLIER_SHARES)]
    items.append((np.ascontiguousarray(np.random.default_rng(5).uniform(0, 1000, (200, 6))), items[0][1]))
    items.append((_contaminated(400, 0.25, 51)[0][:5].copy(), items[0][1]))
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epfl_all.npz"))
    off, K, trip = d["fountain_offsets"], d["fountain_K"], d["fountain_triplets"]
    t = int(np.nonzero(np.diff(off) > 300)[0][0])
    items.append((np.ascontiguousarray(d["fountain_corresp"][off[t]:off[t + 1]]), np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0)))
    assert items[-1][0].shape[0] > 300
    return [a for a, _ in items], np.stack([c for _, c in items])


def _adaptive_dev(method, items, calms, n_hyp, first_round, seed, offsets=None, ns_max=None, **more):
    from tft_vs_fund_amd import api
    packed, off = api.pack_ragged(items)
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.int64)
    out = _ctx().robust_pose_scenes(method, torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(calms)).cuda(),
                                    n_hyp, THR, seed=seed, ns_max=ns_max or max(a.shape[0] for a in items), confidence=CONF, first_round=first_round,
                                    **KW, **more)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}, packed, off


def _one_scene(method, scene, calm, n_hyp, seed):
    out = _ctx().robust_pose(method, torch.from_numpy(scene).cuda(), torch.from_numpy(np.ascontiguousarray(calm)).cuda(), int(n_hyp), THR,
                             seed=seed & ((1 << 64) - 1), **KW)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _assert_scene(out, off, s, ref, what):
    o0, o1 = int(off[s]), int(off[s + 1])
    assert int(out["status"][s]) == int(ref["status"]), (what, s, int(out["status"][s]), int(ref["status"]))
    assert [int(out[k][s]) for k in NAMES] == [int(ref[k]) for k in NAMES], (what, s)
    assert np.array_equal(out["mask"][o0:o1], ref["mask"]), (what, s)
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(out[k][s]), _bits(ref[k])), (what, s, k)


def _rule_in_numpy(method, scene, calm, seed, msac):
    """used[s] from the public pieces: the counts of hypotheses [0, N_HYP), their prefix maxima at the plan's round ends, the rule"""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    n = api.ROBUST_METHODS[method]
    d_scene = torch.from_numpy(scene).cuda(); d_calm = torch.from_numpy(np.ascontiguousarray(calm)).cuda()
    idx = ctx.sample_indices(seed & ((1 << 64) - 1), 0, N_HYP, n, scene.shape[0])
    hyp = ctx.pose_sampled(method, d_scene, d_calm, idx)
    cnt = _np(ctx.inlier_count(d_scene, d_calm, hyp["R_t_2"], hyp["R_t_3"], THR)).astype(np.int64)
    cnt[_np(hyp["status"]) != 0] = -1
    ends, qmin = api.round_plan(CONF, N_HYP, FIRST)
    for e, q in zip(ends, qmin):
        if api.adaptive_stop(int(cnt[:e].max()), scene.shape[0], n, q, msac=msac):
            return int(e)
    return N_HYP


@functools.lru_cache(maxsize=None)
def _shared(method, score):
    """the eight-scene adaptive call (device and host form), the one-scene references at used[s], and used[s] from numpy"""
    ctx = _ctx()
    items, calms = _eight()
    ctx.set_score(score)
    try:
        out, packed, off = _adaptive_dev(method, items, calms, N_HYP, FIRST, SEED)
        host = ctx.robust_pose_scenes(method, packed, off, calms, N_HYP, THR, seed=SEED, confidence=CONF, first_round=FIRST, **KW)
        refs = {s: _one_scene(method, items[s], calms[s], out["n_hyp_used"][s], SEED + s) for s in range(len(items)) if out["n_hyp_used"][s] > 0}
        rule = {s: _rule_in_numpy(method, items[s], calms[s], SEED + s, score == "msac") for s in range(len(items)) if items[s].shape[0] >= 8}
    finally:
        ctx.set_score("count")
    return out, host, off, refs, rule


def _check_contract(method, score):
    from tft_vs_fund_amd import api
    out, host, off, refs, _ = _shared(method, score)
    used = out["n_hyp_used"]
    assert used.dtype == np.int32 and used.shape == (8,)
    assert used[6] == 0 and int(out["status"][6]) == api.ST_TOO_FEW and np.isnan(out["R_t_2"][6]).all() and not out["mask"][off[6]:off[7]].any()
    assert sorted(refs) == [0, 1, 2, 3, 4, 5, 7]
    ends = set(api.round_plan(CONF, N_HYP, FIRST)[0].tolist())
    for s, ref in refs.items():
        assert int(used[s]) in ends, (s, used[s])
        _assert_scene(out, off, s, ref, "%s %s" % (method, score))
    for k in out:                                                             # the _host form
        a, b = out[k], _np(host[k])
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), k


def _check_rule(method, score):
    out, _, _, _, rule = _shared(method, score)
    print("used: library %s, numpy %s" % (out["n_hyp_used"].tolist(), rule))
    for s, e in rule.items():
        assert int(out["n_hyp_used"][s]) == e, (s, int(out["n_hyp_used"][s]), e)
    got = set(rule.values())                                                  # coverage, on the reference's decisions
    assert FIRST in got, "no scene stops after the first round"
    assert N_HYP in got, "no scene runs to the cap"
    assert any(FIRST < e < N_HYP for e in got), "no scene stops strictly in between"


# ---- 1. the contract ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_every_scene_equals_its_one_scene_call_at_used(method):
    _check_contract(method, "count")


# ---- 2. the rule, from public calls ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_used_is_the_rule_on_the_rebuilt_counts(method):
    _check_rule(method, "count")


# ---- 3. MSAC ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_msac(method):
    """the scores rank, and the rule reads best // 64"""
    _check_contract(method, "msac")
    out, _, _, _, rule = _shared(method, "msac")
    print("used: library %s, numpy %s" % (out["n_hyp_used"].tolist(), rule))
    for s, e in rule.items():
        assert int(out["n_hyp_used"][s]) == e, (s, int(out["n_hyp_used"][s]), e)
    assert "score" in out and out["score"].shape == (8,) and out["score"][6] == -1


# ---- 4. a round of more rows than a chunk -------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_a_round_longer_than_a_chunk():
    """five scenes of random matches never stop: round 2 has 5 x 65 536 rows, more than api.ROBUST_CHUNK, and the cuts fall inside scenes"""
    from tft_vs_fund_amd import api
    method = "LinearTFTPoseEstimation"
    rng = np.random.default_rng(9)
    items = [np.ascontiguousarray(rng.uniform(0, 1000, (200, 6))) for _ in range(5)]
    calm = _eight()[1][0]
    assert 5 * 65536 > api.ROBUST_CHUNK
    out, _, off = _adaptive_dev(method, items, calm, 131072, 65536, 77)
    assert out["n_hyp_used"].tolist() == [131072] * 5
    for s in range(5):
        _assert_scene(out, off, s, _one_scene(method, items[s], calm, 131072, 77 + s), "chunks")


# ---- 5. degenerate parameters ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_one_round_is_the_fixed_call(method):
    from tft_vs_fund_amd import api
    items, calms = _eight()
    packed, off = api.pack_ragged(items)
    fixed = _ctx().robust_pose_scenes(method, torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(calms).cuda(), 300, THR,
                                      seed=SEED, ns_max=max(a.shape[0] for a in items), **KW)
    fixed = {k: _np(v) for k, v in fixed.items()}
    assert "n_hyp_used" not in fixed
    for first in (300, 512):                                                  # first_round = n_hyp, and beyond it
        out, _, _ = _adaptive_dev(method, items, calms, 300, first, SEED)
        assert out["n_hyp_used"].tolist() == [300, 300, 300, 300, 300, 300, 0, 300]
        for k, a in fixed.items():
            assert np.array_equal(_bits(a), _bits(out[k])) if a.dtype == np.float64 else np.array_equal(a, out[k]), (first, k)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", METHODS)
def test_bad_offsets_on_the_device(method):
    """scenes 0 and 3 are valid; scene 1 has a decreasing offset, scene 2 more correspondences than ns_max allows"""
    from tft_vs_fund_amd import api
    a, calm = _contaminated(61, 0.25, 11)
    b = _contaminated(40, 0.25, 12)[0]
    big = _contaminated(400, 0.25, 13)[0][:100]
    offsets = [0, 61, 40, 161, 201]                                           # scene 1: 61 -> 40 decreases; scene 2 = [40, 161): 121 > ns_max
    out, _, off = _adaptive_dev(method, [a, big, b], calm, 300, 64, 5, offsets=offsets, ns_max=61)
    used = out["n_hyp_used"]
    assert used[1] == 0 and used[2] == 0 and used[0] > 0 and used[3] > 0
    for s in (1, 2):
        assert int(out["status"][s]) == api.ST_BAD_OFFSETS and np.isnan(out["R_t_2"][s]).all() and np.isnan(out["T"][s]).all()
        assert [int(out[k][s]) for k in NAMES] == [0, -1, 0, 0]
    _assert_scene(out, off, 0, _one_scene(method, a, calm, used[0], 5), "valid 0")
    _assert_scene(out, off, 3, _one_scene(method, b, calm, used[3], 8), "valid 3")
    assert not out["mask"][61:161].any()                                      # nothing was written outside the valid scenes' ranges


@pytest.mark.timeout(300)
def test_refine_and_polish_on_an_adaptive_result():
    """refine= and polish= are the same steps applied by hand to the adaptive result's mask and poses; robust_pose(confidence=) is the S = 1 call"""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    method = "LinearTFTPoseEstimation"
    items, calms = _eight()
    items, calms = items[:3] + items[6:], np.concatenate([calms[:3], calms[6:]])       # noise-free, 20 %, 35 %, the scene of 5 matches, the fountain triplet
    plain, packed, off = _adaptive_dev(method, items, calms, N_HYP, FIRST, SEED)
    out, _, _ = _adaptive_dev(method, items, calms, N_HYP, FIRST, SEED, refine="OptimFPoseEstimation", polish=True)
    for k, a in plain.items():
        assert np.array_equal(_bits(a), _bits(out[k])) if a.dtype == np.float64 else np.array_equal(a, out[k]), k
    keep = plain["mask"] != 0
    cum = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
    r = ctx.pose_batch_ragged("OptimFPoseEstimation", torch.from_numpy(np.ascontiguousarray(packed[keep])).cuda(), torch.from_numpy(cum[off]).cuda(),
                              torch.from_numpy(calms).cuda(), reconst=False)
    ba = ctx.bundle_adjust_ragged(torch.from_numpy(calms).cuda(), torch.from_numpy(plain["R_t_2"]).cuda(), torch.from_numpy(plain["R_t_3"]).cuda(),
                                  torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), mask=torch.from_numpy(plain["mask"]).cuda(), reconst=False)
    torch.cuda.synchronize()
    for k, v in (("R_t_2_refined", r["R_t_2"]), ("R_t_3_refined", r["R_t_3"]), ("T_refined", r["T"]), ("R_t_2_polished", ba["R_t_2"]),
                 ("R_t_3_polished", ba["R_t_3"]), ("repr_err_polished", ba["repr_err"])):
        assert np.array_equal(_bits(out[k]), _bits(v)), k
    for k, v in (("iter_refined", r["iter"]), ("status_refined", r["status"]), ("iter_polished", ba["iter"]), ("status_polished", ba["status"])):
        assert np.array_equal(out[k], _np(v)), k
    assert (out["status_refined"][[0, 1, 2, 4]] == 0).all() and out["status_refined"][3] == api.ST_TOO_FEW
    # robust_pose with a confidence: scene 1 of the list alone, with its seed
    one = ctx.robust_pose(method, torch.from_numpy(items[1]).cuda(), torch.from_numpy(calms[1]).cuda(), N_HYP, THR, seed=SEED + 1, confidence=CONF,
                          first_round=FIRST, **KW)
    torch.cuda.synchronize()
    assert int(one["n_hyp_used"]) == int(plain["n_hyp_used"][1]) and one["R_t_2"].shape == (3, 4) and one["T"].shape == (3, 3, 3)
    _assert_scene(plain, off, 1, {k: _np(v) for k, v in one.items()}, "robust_pose(confidence=)")
    h = ctx.robust_pose(method, items[1], calms[1], N_HYP, THR, seed=SEED + 1, confidence=CONF, first_round=FIRST, **KW)
    assert isinstance(h["n_hyp_used"], int) and h["n_hyp_used"] == int(plain["n_hyp_used"][1]) and h["status"] == 0
    assert np.array_equal(_bits(h["R_t_2"]), _bits(one["R_t_2"])) and np.array_equal(h["mask"], _np(one["mask"]))
