"""
Covariances of the three-view bundle adjustment on the GPU (tff_ba_covariance_*, tff_bundle_adjust_cov_*, Context.ba_covariance,
Context.ba_covariance_ragged, cov= / point_cov= of bundle_adjust and bundle_adjust_ragged, polish_cov= of the robust estimators; include/tftfund_cov.h).

  1. the kernel against the numpy restatement (tests/ba_cov_oracle.py) at the restatement's own optimum: the cases and the gates of
     tests/test_emulated_ba_cov.py, at B = 1 and at B = 7 with a CalM per item, item results bit-equal between the two;
  2. the ragged call against the fixed-N call, bit for bit; the host form against the device form;
  3. the adjustment with cov=True: every other output keeps its bits, and cov, sigma0, point_cov are ba_covariance on its outputs.  (The adjustment's
     covariance against the restatement's at the restatement's optimum would need a looser gate -- 1e-9 in the parameters moves the covariance by
     3e-9 .. 1e-7, 2e-6 at N = 4 --; the composition avoids that comparison);
  4. Monte Carlo on the device: 2048 noise draws of one scene in one call, empirical against predicted standard deviations;
  5. the robust calls with polish_cov=True.
"""
import functools
import os

import numpy as np
import pytest

import ba_cov_cases as cc
import ba_loss_cases as bc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@functools.lru_cache(maxsize=None)
def _ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    return api.Context(0)


def _np(out):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b, keys):
    for k in keys:
        assert cc.biteq(a[k], b[k]), k


def _fixed(C, CalM, Rt2, Rt3, X, loss, c):
    """Context.ba_covariance with B = 1: C (n, 6), Rt 3x4, X (n, 3) -> cov (144,), sigma0, point_cov (n, 6)"""
    o = _np(_ctx().ba_covariance(CalM, Rt2[None], Rt3[None], np.ascontiguousarray(C)[None], np.ascontiguousarray(X.T)[None], loss=loss, scale=c, point_cov=True))
    return o["cov"][0].reshape(144), float(o["sigma0"][0]), o["point_cov"][0]


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_bad,loss,c", cc.CASES)
def test_kernel_matches_the_restatement(n, n_bad, loss, c):
    sc = bc.scene(n, n_bad)
    R_t, X = (np.array(a) for a in cc.optimum(n, n_bad, loss, c))              # (copies: the cached arrays are read-only)
    cov, s0, pc = _fixed(sc["C"], sc["CalM"], R_t[3:6], R_t[6:9], X.T, loss, c)
    cc.gate(cc.reference(n, n_bad, loss, c), cov.reshape(12, 12), s0, pc, (n, n_bad, loss, c))
    B = 7
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))
    o = _np(_ctx().ba_covariance(rep(sc["CalM"]), rep(R_t[3:6]), rep(R_t[6:9]), rep(sc["C"]), rep(np.asarray(X)), loss=loss, scale=c, point_cov=True))
    for b in range(B):
        assert cc.biteq(o["cov"][b].reshape(144), cov) and o["sigma0"][b] == s0 and cc.biteq(o["point_cov"][b], pc), b
    bare = _np(_ctx().ba_covariance(rep(sc["CalM"]), rep(R_t[3:6]), rep(R_t[6:9]), rep(sc["C"]), rep(np.asarray(X)), loss=loss, scale=c))
    assert "point_cov" not in bare
    _same(bare, o, ("cov", "sigma0"))


@pytest.mark.parametrize("loss,c", cc.LOSSES[0:2])
def test_no_redundancy_and_bad_poses_give_nan(loss, c):
    sc = bc.scene(12, 0)
    for C, Rt2, X in ((sc["C"][:3], sc["start"][0], sc["X0"][:3]), (sc["C"], sc["start"][0] * np.nan, sc["X0"])):
        cov, s0, pc = _fixed(C, sc["CalM"], Rt2, sc["start"][1], X, loss, c)
        assert np.isnan(cov).all() and np.isnan(s0) and np.isnan(pc).all()


# ---- 2. ragged equals fixed-N -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,c", (("huber", 3.0), (None, None)))
def test_ragged_items_equal_the_fixed_call(loss, c):
    ctx = _ctx()
    rc = cc.ragged_case()
    B, nt = len(rc["sizes"]), rc["nt"]
    scs = rc["scs"]
    calm = np.stack([s["CalM"] for s in scs]); r2 = np.stack([s["start"][0] for s in scs]); r3 = np.stack([s["start"][1] for s in scs])
    fixed = lambda b, sel: _fixed(scs[b]["C"][sel], scs[b]["CalM"], scs[b]["start"][0], scs[b]["start"][1], scs[b]["X0"][sel], loss, c)
    ok = rc["off"].copy(); ok[-1] = nt                                         # the same batch with a valid last item, for the host form
    for mk in (rc["mask"], None):
        o = _np(ctx.ba_covariance_ragged(_cu(calm), _cu(r2), _cu(r3), _cu(rc["packed"]), _cu(rc["off"]), _cu(rc["X"]), mask=_cu(mk), loss=loss, scale=c,
                                         point_cov=True))
        pc = np.concatenate([o["point_cov"], np.full((4, 6), 5.0)])
        pc[int(rc["off"][-2]):nt] = 5.0 if np.isnan(o["point_cov"][int(rc["off"][-2]):nt]).all() else 7.0   # (the wrapper presets NaN: an item without a range keeps it)
        cc.check_ragged(rc, mk, o["cov"].reshape(B, 144), o["sigma0"], pc, fixed)
        bare = _np(ctx.ba_covariance_ragged(_cu(calm), _cu(r2), _cu(r3), _cu(rc["packed"]), _cu(rc["off"]), _cu(rc["X"]), mask=_cu(mk), loss=loss, scale=c))
        _same(bare, o, ("cov", "sigma0"))
        dev = _np(ctx.ba_covariance_ragged(_cu(calm), _cu(r2), _cu(r3), _cu(rc["packed"]), _cu(ok), _cu(rc["X"]), mask=_cu(mk), loss=loss, scale=c, point_cov=True))
        host = ctx.ba_covariance_ragged(calm, r2, r3, rc["packed"], ok, rc["X"], mask=mk, loss=loss, scale=c, point_cov=True)
        _same(host, dev, ("cov", "sigma0", "point_cov"))
        for b in range(B - 1):                                                 # the neighbours of the bad item: the same bits with and without it
            assert cc.biteq(dev["cov"][b], o["cov"][b]), b
        assert np.isfinite(dev["cov"][B - 1]).all()


# ---- 3. the adjustment with its covariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,c", ((None, None), ("cauchy", 3.0)))
def test_bundle_adjust_with_cov_is_the_adjustment_then_the_covariance(loss, c):
    ctx = _ctx()
    scs = [bc.scene(65, 13, seed=310 + k, focalL=40.0 + 4.0 * k) for k in range(3)]
    calm = np.stack([s["CalM"] for s in scs]); s2 = np.stack([s["start"][0] for s in scs]); s3 = np.stack([s["start"][1] for s in scs])
    C = np.stack([s["C"] for s in scs])
    plain = _np(ctx.bundle_adjust(calm, s2, s3, C, loss=loss, scale=c))
    full = _np(ctx.bundle_adjust(calm, s2, s3, C, loss=loss, scale=c, cov=True, point_cov=True))
    keys = ("R_t_2", "R_t_3", "Reconst", "repr_err") + (("weight",) if loss else ())
    _same(full, plain, keys)
    assert np.array_equal(full["iter"], plain["iter"]) and np.array_equal(full["status"], plain["status"]) and (full["status"] == 0).all()
    assert full["cov"].shape == (3, 12, 12) and full["sigma0"].shape == (3,) and full["point_cov"].shape == (3, 65, 6)
    again = _np(ctx.ba_covariance(calm, full["R_t_2"], full["R_t_3"], C, full["Reconst"], loss=loss, scale=c, point_cov=True))
    _same(full, again, ("cov", "sigma0", "point_cov"))
    only = _np(ctx.bundle_adjust(calm, s2, s3, C, loss=loss, scale=c, cov=True))
    assert "point_cov" not in only
    _same(only, full, keys + ("cov", "sigma0"))
    assert np.isfinite(full["cov"]).all() and (full["sigma0"] > 0).all()
    rot = _ctx_api().euler_cov_to_rotvec(full["R_t_2"], full["R_t_3"], full["cov"])
    deg = np.degrees(np.sqrt(np.trace(rot[:, 0:3, 0:3], axis1=1, axis2=2)))
    print("rotation sigma of view 2, degrees:", deg)
    assert np.isfinite(deg).all() and (deg > 0).all()


def _ctx_api():
    from tft_vs_fund_amd import api
    return api


@pytest.mark.parametrize("loss,c", ((None, None), ("huber", 3.0)))
def test_bundle_adjust_ragged_with_cov_is_the_adjustment_then_the_covariance(loss, c):
    ctx = _ctx()
    rc = cc.ragged_case()
    B, nt = len(rc["sizes"]), rc["nt"]
    scs = rc["scs"]
    calm = np.stack([s["CalM"] for s in scs]); r2 = np.stack([s["start"][0] for s in scs]); r3 = np.stack([s["start"][1] for s in scs])
    off = rc["off"].copy(); off[-1] = nt
    a = (_cu(calm), _cu(r2), _cu(r3), _cu(rc["packed"]), _cu(off))
    kw = dict(mask=_cu(rc["mask"]), reconst0=_cu(rc["X"]), loss=loss, scale=c)
    plain = _np(ctx.bundle_adjust_ragged(*a, **kw))
    full = _np(ctx.bundle_adjust_ragged(*a, cov=True, point_cov=True, **kw))
    keys = ("R_t_2", "R_t_3", "Reconst", "repr_err") + (("weight",) if loss else ())
    _same(full, plain, keys)
    for k in ("iter", "status", "used"):
        assert np.array_equal(full[k], plain[k]), k
    again = _np(ctx.ba_covariance_ragged(a[0], _cu(full["R_t_2"]), _cu(full["R_t_3"]), a[3], a[4], _cu(full["Reconst"]), mask=kw["mask"], loss=loss, scale=c,
                                         point_cov=True))
    _same(full, again, ("cov", "sigma0", "point_cov"))
    ok = np.array(rc["keep"]) > 3
    assert np.isfinite(full["cov"][ok]).all() and np.isnan(full["cov"][~ok]).all() and np.isnan(full["sigma0"][~ok]).all()
    # without a `reconst` output the points live in the context; the host form
    lean = _np(ctx.bundle_adjust_ragged(*a, reconst=False, cov=True, **kw))
    assert lean["Reconst"] is None
    _same(lean, full, ("R_t_2", "R_t_3", "repr_err", "cov", "sigma0"))
    host = ctx.bundle_adjust_ragged(calm, r2, r3, rc["packed"], off, mask=rc["mask"], reconst0=rc["X"], loss=loss, scale=c, cov=True, point_cov=True)
    _same(host, full, keys + ("cov", "sigma0", "point_cov"))


# ---- 4. Monte Carlo ---------------------------------------------------------------------------------------------------------------------------------------
def test_predicted_covariance_is_the_scatter_of_2048_adjustments():
    """one bundle_adjust(cov=True) call on B = 2048 draws of 1 px noise around the noiseless matches of the scene of tests/test_ba_cov_cpu.py, each
    from the truth: every item converges (status 0), and the standard deviation of each of the twelve returned parameters over the mean predicted
    one is 1 within 0.08 (5 / sqrt(2 B) = 0.078: five standard errors of a standard deviation from B samples)"""
    B = 2048
    ms = cc.mc_scene()
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))
    o = _np(_ctx().bundle_adjust(ms["CalM"], rep(ms["truth"][0]), rep(ms["truth"][1]), cc.mc_draws(B), rep(ms["X"].T), cov=True))
    assert (o["status"] == 0).all()
    ratio = cc.mc_ratio(cc.mc_params(o["R_t_2"], o["R_t_3"]), o["cov"])
    print("empirical / predicted standard deviation:", np.round(ratio, 3), "iterations:", o["iter"].min(), "..", o["iter"].max())
    assert np.abs(ratio - 1.0).max() <= 0.08, ratio


# ---- 5. the robust calls -----------------------------------------------------------------------------------------------------------------------------------
def _synthetic(n, gen_seed):
    """0.5 px noise, 30 % of the matches displaced by U(20, 80) px in views 2, 3"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, n, noise=0.5, seed=gen_seed)
    scene = C[0].copy()
    rng = np.random.default_rng(gen_seed + 100)
    bad = rng.choice(n, (3 * n) // 10, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    return np.ascontiguousarray(scene), np.ascontiguousarray(CalM)


@pytest.mark.parametrize("kw", (dict(), dict(polish_loss="cauchy", polish_all=True)), ids=("mask", "cauchy_all"))
def test_robust_calls_with_polish_cov(kw):
    """five synthetic scenes at 30 % outliers, the first too small to give a pose"""
    api = _ctx_api()
    ctx = _ctx()
    method, n_hyp, thr, seed = "LinearTFTPoseEstimation", 300, 4.0, 21
    pairs = [_synthetic(n, 60 + k) for k, n in enumerate((5, 61, 100, 150, 240))]
    packed, off = api.pack_ragged([a for a, _ in pairs])
    calms = np.stack([c for _, c in pairs])
    S = len(pairs)
    call = lambda **more: _np(ctx.robust_pose_scenes(method, _cu(packed), _cu(off), _cu(calms), n_hyp, thr, seed=seed, ns_max=int(np.diff(off).max()), polish=True,
                                                     **kw, **more))
    base, out = call(), call(polish_cov=True)
    assert set(out) - set(base) == {"cov_polished", "sigma0_polished"}
    for k in base:                                                             # every existing key keeps its bits
        assert np.array_equal(np.asarray(out[k]), np.asarray(base[k]), equal_nan=True) and (out[k].dtype != np.float64 or cc.biteq(out[k], base[k])), k
    assert out["cov_polished"].shape == (S, 12, 12) and out["sigma0_polished"].shape == (S,)
    # by hand: the polish call with its points, then the covariance at them
    mask = None if kw.get("polish_all") else _cu(out["mask"])
    how = dict(loss=kw.get("polish_loss"), scale=thr if kw else None)
    hand = _np(ctx.bundle_adjust_ragged(_cu(calms), _cu(out["R_t_2"]), _cu(out["R_t_3"]), _cu(packed), _cu(off), mask=mask, **how))
    assert cc.biteq(hand["R_t_2"], out["R_t_2_polished"]) and cc.biteq(hand["R_t_3"], out["R_t_3_polished"])
    cov = _np(ctx.ba_covariance_ragged(_cu(calms), _cu(hand["R_t_2"]), _cu(hand["R_t_3"]), _cu(packed), _cu(off), _cu(hand["Reconst"]), mask=mask, **how))
    assert cc.biteq(cov["cov"], out["cov_polished"]) and cc.biteq(cov["sigma0"], out["sigma0_polished"])
    assert out["status"][0] != 0 and np.isnan(out["cov_polished"][0]).all() and np.isnan(out["sigma0_polished"][0])
    assert (out["status"][1:] == 0).all() and (out["status_polished"][1:] == 0).all()
    assert np.isfinite(out["cov_polished"][1:]).all() and (out["sigma0_polished"][1:] > 0).all()
    # the numpy form, and one scene through robust_pose with seed + s
    host = ctx.robust_pose_scenes(method, packed, off, calms, n_hyp, thr, seed=seed, polish=True, polish_cov=True, **kw)
    assert cc.biteq(host["cov_polished"], out["cov_polished"]) and cc.biteq(host["sigma0_polished"], out["sigma0_polished"])
    s = 2
    one = _np(ctx.robust_pose(method, _cu(pairs[s][0]), _cu(pairs[s][1]), n_hyp, thr, seed=seed + s, polish=True, polish_cov=True, **kw))
    assert one["cov_polished"].shape == (12, 12)
    assert cc.biteq(one["cov_polished"], out["cov_polished"][s]) and cc.biteq(one["sigma0_polished"], out["sigma0_polished"][s])
    assert cc.biteq(one["R_t_2_polished"], out["R_t_2_polished"][s])


# ---- 6. the fixed-N host forms (no Python wrapper takes them) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,c", ((None, None), ("huber", 3.0)))
def test_batch_host_forms_equal_the_device_forms(loss, c):
    import ctypes
    api = _ctx_api()
    ctx = _ctx()
    scs = [bc.scene(40, 2, seed=320 + k, focalL=40.0 + 4.0 * k) for k in range(3)]
    B, N = 3, 40
    calm = np.stack([s["CalM"] for s in scs]); s2 = np.stack([s["start"][0] for s in scs]); s3 = np.stack([s["start"][1] for s in scs])
    C = np.ascontiguousarray(np.stack([s["C"] for s in scs]))
    dev = _np(ctx.bundle_adjust(calm, s2, s3, C, loss=loss, scale=c, cov=True, point_cov=True))
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    cm = lambda Rt: np.ascontiguousarray(Rt.transpose(0, 2, 1)).reshape(B, 12)
    calm_cm, r2, r3 = np.ascontiguousarray(calm.transpose(0, 2, 1)).reshape(B * 27), cm(s2), cm(s3)
    lid, sc_ = api.LOSS_IDS.get(loss, 0), float(c or 0.0)
    for with_rec in (True, False):                                             # without a reconst output the call keeps the points itself
        o2, o3, rec = np.zeros((B, 12)), np.zeros((B, 12)), np.zeros((B, N, 3)) if with_rec else None
        it, st, err = np.zeros(B, dtype=np.int32), np.full(B, -7, dtype=np.int32), np.zeros(B)
        w = np.zeros((B, N)) if loss else None
        cov, s0, pc = np.zeros((B, 12, 12)), np.zeros(B), np.zeros((B, N, 6))
        assert ctx.lib.tff_bundle_adjust_cov_batch_host(ctx.handle, P(calm_cm), 27, P(r2), P(r3), P(C), B, N, None, P(o2), P(o3), P(rec), P(it), P(err), P(st), lid, sc_,
                                                        P(w), P(cov), P(s0), P(pc)) == 0
        assert (st == 0).all() and np.array_equal(it, dev["iter"])
        assert cc.biteq(o2.reshape(B, 4, 3).transpose(0, 2, 1), dev["R_t_2"]) and cc.biteq(err, dev["repr_err"])
        assert cc.biteq(cov, dev["cov"]) and cc.biteq(s0, dev["sigma0"]) and cc.biteq(pc, dev["point_cov"])
        assert loss is None or cc.biteq(w, dev["weight"])
    cov2, s02 = np.zeros((B, 12, 12)), np.zeros(B)                             # the covariance alone, at those outputs, without the point blocks
    X = np.ascontiguousarray(dev["Reconst"].transpose(0, 2, 1))                # (named: a pointer does not keep its array alive)
    assert ctx.lib.tff_ba_covariance_batch_host(ctx.handle, P(calm_cm), 27, P(o2), P(o3), P(C), B, N, P(X), lid, sc_, P(cov2), P(s02), None) == 0
    assert cc.biteq(cov2, dev["cov"]) and cc.biteq(s02, dev["sigma0"])
    assert ctx.lib.tff_ba_covariance_batch_host(ctx.handle, P(calm_cm), 27, P(o2), P(o3), P(C), B, N, None, lid, sc_, P(cov2), P(s02), None) == -10001   # reconst is required
