"""
The covariance of the bundle adjustment over tracks on the GPU (tff_ba_tracks_covariance_batch_dev / _host, tff_bundle_adjust_tracks_cov_batch_dev /
_host, include/tftfund_tracks_cov.h; Context.ba_tracks_covariance and Context.bundle_adjust_views(..., cov=True)) against the numpy restatement
(tests/ba_tracks_cov_oracle.py) over the cases of tests/ba_tracks_cov_cases.py at its gate.  All cases of one (M, loss) go into ONE call, NaN-padded to
N = 130: the padding contract is thereby tested on every case.  Bit for bit: _host and _dev, an item alone and inside the padded batch, with and
without point_cov, the combined call against the adjustment followed by the stand-alone covariance.  The three-view call on fully visible three-view
input, the items without a covariance, every TFF_E_INVALID, and the scatter of 2 048 adjustments against the predicted covariance.
"""
import ctypes
import functools

import numpy as np
import pytest

import ba_tracks_cases as tc
import ba_tracks_cov_cases as tcc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
D = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
NPAD = tcc.N_PAD
E_INVALID = -10001
biteq = tcc.biteq


@functools.lru_cache(maxsize=None)
def _ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    return api.Context(0)


def _item(k, pad=NPAD):
    """case k at the restatement's final parameters -> (CalM, R_t 3M x 4, C (pad, 2M), X (pad, 3))"""
    CalM, _, C, _ = tcc.inputs(*k[0:4])
    R_t, X = tcc.optimum(*k)
    Cp, Xp = tcc.padded(C, X, C.shape[1] if pad is None else pad)
    return CalM, R_t, Cp, Xp


def _arrays(items):
    M = items[0][2].shape[1] // 2
    calm = np.ascontiguousarray(items[0][0].T).reshape(-1)
    rt = np.stack([np.ascontiguousarray(i[1].T).reshape(-1) for i in items]); Cc = np.stack([i[2] for i in items]); X = np.stack([i[3] for i in items])
    return M, calm, rt, Cc, X


def _host(items, loss, c, points=True):
    """tff_ba_tracks_covariance_batch_host on items of one M and one N -> cov (B,P,P), sigma0 (B,), point_cov (B,N,6) or None"""
    ctx = _ctx()
    M, calm, rt, Cc, X = _arrays(items)
    B, N = Cc.shape[0:2]; Pn = 6 * (M - 1)
    cov = np.full((B, Pn, Pn), 5.0); s0 = np.full(B, 5.0); pc = np.full((B, N, 6), 5.0) if points else None
    assert ctx.lib.tff_ba_tracks_covariance_batch_host(ctx.handle, M, P(calm), 0, P(rt), P(Cc), B, N, P(X), tcc.LOSS_ID[loss], float(c or 0.0), P(cov), P(s0), P(pc)) == 0
    return cov, s0, pc


def _dev(items, loss, c, points=True):
    ctx = _ctx()
    M, calm, rt, Cc, X = _arrays(items)
    B, N = Cc.shape[0:2]; Pn = 6 * (M - 1)
    t = [torch.from_numpy(a).cuda() for a in (calm, rt, Cc, X)]
    cov = torch.full((B, Pn, Pn), 5.0, dtype=torch.float64, device="cuda"); s0 = torch.full((B,), 5.0, dtype=torch.float64, device="cuda")
    pc = torch.full((B, N, 6), 5.0, dtype=torch.float64, device="cuda") if points else None
    assert ctx.lib.tff_ba_tracks_covariance_batch_dev(ctx.handle, M, D(t[0]), 0, D(t[1]), D(t[2]), B, N, D(t[3]), tcc.LOSS_ID[loss], float(c or 0.0), D(cov), D(s0), D(pc)) == 0
    torch.cuda.synchronize()
    return cov.cpu().numpy(), s0.cpu().numpy(), pc.cpu().numpy() if points else None


def _group(M, loss, c):
    return [k for k in tcc.CASES if k[0] == M and k[3:] == (loss, c)]


GROUPS = [(M, loss, c) for M in tcc.VIEWS for loss, c in tcc.LOSSES]


def test_the_groups_cover_every_case():
    assert sorted((k for g in GROUPS for k in _group(*g)), key=repr) == sorted(tcc.CASES, key=repr)
    assert len(tcc.LEFT_OUT) <= len(tcc.CASES) // 10 and not [k for k in tcc.LEFT_OUT if k[2] == "full"]


@pytest.mark.parametrize("M,loss,c", GROUPS)
def test_every_case_matches_the_restatement_dev_and_host(M, loss, c):
    keys = _group(M, loss, c)
    items = [_item(k) for k in keys]
    dev, host = _dev(items, loss, c), _host(items, loss, c)
    assert biteq(dev[0], host[0]) and biteq(dev[1], host[1]) and biteq(dev[2], host[2])        # the same kernel on the same bytes
    no_pc = _dev(items, loss, c, points=False)
    assert biteq(no_pc[0], dev[0]) and biteq(no_pc[1], dev[1])                                  # point_cov = NULL: the same cov bits
    for b, k in enumerate(keys):
        N = k[1]
        assert np.isnan(dev[2][b][N:]).all(), k                                                 # the padding rows: NaN
        tcc.gate(tcc.reference(*k), dev[0][b], float(dev[1][b]), dev[2][b][:N], k, full=k not in tcc.LEFT_OUT)


@pytest.mark.parametrize("M,N", [(3, 65), (6, 130)])
@pytest.mark.parametrize("loss,c", tcc.LOSSES)
def test_an_item_alone_equals_the_item_in_the_padded_batch(M, N, loss, c):
    keys = _group(M, loss, c)
    batch = _dev([_item(k) for k in keys], loss, c)
    k = (M, N, "random", loss, c)
    b = keys.index(k)
    for run in (_dev, _host):
        alone = run([_item(k, pad=None)], loss, c)
        assert alone[2].shape == (1, N, 6)
        assert biteq(alone[0][0], batch[0][b]) and biteq(alone[1][0:1], batch[1][b:b + 1]) and biteq(alone[2][0], batch[2][b][:N]), (k, run.__name__)
    # ... and through the wrapper
    CalM, R_t, Cp, Xp = _item(k, pad=None)
    out = _ctx().ba_tracks_covariance(CalM, R_t[None], Cp[None], np.ascontiguousarray(Xp.T)[None], loss=loss, scale=c, point_cov=True)
    torch.cuda.synchronize()
    assert biteq(out["cov"].cpu().numpy()[0], batch[0][b]) and biteq(out["point_cov"].cpu().numpy()[0], batch[2][b][:N])


def _adjust_host(fn_name, M, case, loss, c, cov_args=()):
    """a tracks adjustment through a _host entry point, B = 1, every output requested -> dict of outputs"""
    ctx = _ctx()
    CalM, R0, C, X0 = case
    N = C.shape[1]
    calm = np.ascontiguousarray(CalM.T).reshape(-1); rt = np.ascontiguousarray(R0.T).reshape(1, -1); Cc = np.ascontiguousarray(C.T)[None]
    x0 = np.ascontiguousarray(X0.T)[None] if X0 is not None else None
    o = dict(Rt=np.full((1, 12 * M), 5.0), rec=np.full((1, N, 3), 5.0), it=np.full(1, 5, dtype=np.int32), err=np.full(1, 5.0), used=np.full(1, -5, dtype=np.int32),
             st=np.full(1, 5, dtype=np.int32), w=np.full((1, N, M), 5.0))
    assert getattr(ctx.lib, fn_name)(ctx.handle, M, P(calm), 0, P(rt), P(Cc), 1, N, P(x0), P(o["Rt"]), P(o["rec"]), P(o["it"]), P(o["err"]), P(o["used"]), P(o["st"]),
                                     tcc.LOSS_ID[loss], float(c or 0.0), P(o["w"]), *cov_args) == 0
    return o


@pytest.mark.parametrize("M,N,pattern", [(3, 65, "random"), (6, 130, "few_obs"), (4, 64, "view_nan")])
@pytest.mark.parametrize("loss,c", tcc.LOSSES)
def test_the_combined_call_is_the_adjustment_followed_by_the_covariance(M, N, pattern, loss, c):
    ctx = _ctx()
    case = tcc.inputs(M, N, pattern, loss)
    Pn = 6 * (M - 1)
    plain = _adjust_host("tff_bundle_adjust_tracks_loss_batch_host", M, case, loss, c)
    cov = np.full((1, Pn, Pn), 5.0); s0 = np.full(1, 5.0); pc = np.full((1, N, 6), 5.0)
    both = _adjust_host("tff_bundle_adjust_tracks_cov_batch_host", M, case, loss, c, (P(cov), P(s0), P(pc)))
    for key in plain:                                                        # every adjustment output keeps its bits
        assert plain[key].tobytes() == both[key].tobytes(), key
    assert int(plain["st"][0]) == 0
    R_t = plain["Rt"][0].reshape(4, 3 * M).T
    want = _host([(case[0], R_t, np.ascontiguousarray(case[2].T), plain["rec"][0])], loss, c)
    assert biteq(cov, want[0]) and biteq(s0, want[1]) and biteq(pc, want[2])
    assert np.isfinite(cov).all() and s0[0] > 0.0
    # the _dev form through the wrapper: the same bits, with the points kept by the caller ...
    X0 = None if case[3] is None else case[3][None]
    out = ctx.bundle_adjust_views(case[0], case[1][None], np.ascontiguousarray(case[2].T)[None], X0, missing="point", loss=loss, scale=c, cov=True, point_cov=True)
    torch.cuda.synchronize()
    assert np.ascontiguousarray(out["R_t"].cpu().numpy()[0]).tobytes() == np.ascontiguousarray(R_t).tobytes() and int(out["iter"][0]) == int(plain["it"][0])
    assert biteq(out["cov"].cpu().numpy(), cov) and biteq(out["sigma0"].cpu().numpy(), s0) and biteq(out["point_cov"].cpu().numpy(), pc)
    assert ("weight" in out) == (loss is not None)
    # ... and with reconst == NULL, in a workspace of the context
    t = [torch.from_numpy(a).cuda() for a in (np.ascontiguousarray(case[0].T).reshape(-1), np.ascontiguousarray(case[1].T).reshape(1, -1), np.ascontiguousarray(case[2].T)[None])]
    x0 = torch.from_numpy(np.ascontiguousarray(case[3].T)[None]).cuda() if case[3] is not None else None
    o = torch.empty((1, 12 * M), dtype=torch.float64, device="cuda")
    cv = torch.empty((1, Pn, Pn), dtype=torch.float64, device="cuda"); sg = torch.empty(1, dtype=torch.float64, device="cuda")
    assert ctx.lib.tff_bundle_adjust_tracks_cov_batch_dev(ctx.handle, M, D(t[0]), 0, D(t[1]), D(t[2]), 1, N, D(x0), D(o), None, None, None, None, None,
                                                          tcc.LOSS_ID[loss], float(c or 0.0), None, D(cv), D(sg), None) == 0
    torch.cuda.synchronize()
    assert biteq(cv.cpu().numpy(), cov) and biteq(sg.cpu().numpy(), s0) and o.cpu().numpy().tobytes() == plain["Rt"].tobytes()


@pytest.mark.parametrize("N", (12, 65, 130))
def test_fully_visible_three_views_agree_with_the_three_view_call(N):
    ctx = _ctx()
    k = (3, N, "full", None, None)
    CalM, R_t, Cp, Xp = _item(k, pad=None)
    got = _dev([(CalM, R_t, Cp, Xp)], None, None)
    out = ctx.ba_covariance(CalM, R_t[None, 3:6], R_t[None, 6:9], Cp[None], np.ascontiguousarray(Xp.T)[None], point_cov=True)
    torch.cuda.synchronize()
    cov3, s03, pc3 = out["cov"].cpu().numpy()[0], float(out["sigma0"][0]), out["point_cov"].cpu().numpy()[0]
    figs = (np.abs(got[0][0] - cov3).max() / np.abs(cov3).max(), abs(got[1][0] - s03) / s03, (np.abs(got[2][0] - pc3).max(axis=1) / np.abs(pc3).max(axis=1)).max())
    print(k, figs)
    assert max(figs) <= 1e-9, figs


@pytest.mark.parametrize("loss,c", tcc.LOSSES)
def test_failing_items_between_two_good_ones(loss, c):
    for kind in tcc.FAILING:
        M, CalM, R_t, C, X = tcc.failing(kind)
        N = C.shape[1]
        goods = [_item((M, 12, p, loss, c), pad=None) for p in (("full", "few_obs") if M == 2 else ("random", "full"))]
        Cf, Xf = tcc.padded(C, X, 12)
        batch = [goods[0], (CalM, R_t, Cf, Xf), goods[1]]
        for run in (_dev, _host):
            cov, s0, pc = run(batch, loss, c)
            assert np.isnan(cov[1]).all() and np.isnan(s0[1]) and np.isnan(pc[1]).all(), (kind, run.__name__)
            for b, g in ((0, goods[0]), (2, goods[1])):                       # the neighbours keep the bits they have alone
                alone = run([g], loss, c)
                assert np.isfinite(alone[0]).all() and alone[1][0] > 0.0
                assert biteq(cov[b], alone[0][0]) and biteq(s0[b:b + 1], alone[1]) and biteq(pc[b], alone[2][0]), (kind, b, run.__name__)


def test_every_invalid_argument_is_refused_before_any_work():
    ctx = _ctx()
    M, N, B = 3, 12, 1
    CalM, R_t, Cp, Xp = _item((M, N, "full", None, None), pad=None)
    calm = np.ascontiguousarray(CalM.T).reshape(-1); rt = np.ascontiguousarray(R_t.T).reshape(-1)
    Pn = 6 * (M - 1)
    cov = np.full(Pn * Pn, 5.0); s0 = np.full(1, 5.0); pc = np.full((N, 6), 5.0); o = np.full(12 * M, 5.0)
    untouched = lambda: cov.tobytes() == np.full(Pn * Pn, 5.0).tobytes() and s0[0] == 5.0 and pc.tobytes() == np.full((N, 6), 5.0).tobytes() and o.tobytes() == np.full(12 * M, 5.0).tobytes()
    good = dict(M=M, calm=P(calm), stride=0, rt=P(rt), C=P(Cp), B=B, N=N, X=P(Xp), out=P(o), loss=1, scale=1.5, cov=P(cov), s0=P(s0))
    refused = [dict(loss=3), dict(loss=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(loss=2, scale=0.0),
               dict(M=1), dict(M=7), dict(B=-1), dict(N=-1), dict(N=0), dict(calm=None), dict(rt=None), dict(C=None), dict(stride=5), dict(loss=0, M=7),
               dict(loss=0, calm=None), dict(cov=None), dict(s0=None)]
    for suffix in ("host", "dev"):
        alone = getattr(ctx.lib, "tff_ba_tracks_covariance_batch_" + suffix)
        both = getattr(ctx.lib, "tff_bundle_adjust_tracks_cov_batch_" + suffix)
        for ch in refused + [dict(X=None)]:                                  # the stand-alone form: reconst is required
            a = dict(good); a.update(ch)
            r = alone(ctx.handle, a["M"], a["calm"], a["stride"], a["rt"], a["C"], a["B"], a["N"], a["X"], a["loss"], a["scale"], a["cov"], a["s0"], P(pc))
            assert r == E_INVALID and len(ctx.lib.tff_last_error()) > 0 and untouched(), (alone.__name__, ch)
        for ch in refused + [dict(out=None)]:
            a = dict(good); a.update(ch)
            r = both(ctx.handle, a["M"], a["calm"], a["stride"], a["rt"], a["C"], a["B"], a["N"], None, a["out"], None, None, None, None, None, a["loss"], a["scale"], None,
                     a["cov"], a["s0"], P(pc))
            assert r == E_INVALID and len(ctx.lib.tff_last_error()) > 0 and untouched(), (both.__name__, ch)
        assert alone(None, M, P(calm), 0, P(rt), P(Cp), B, N, P(Xp), 0, 0.0, P(cov), P(s0), P(pc)) == E_INVALID
        assert ctx.lib.tff_last_error().decode() == "null context"
        # B = 0 is a call that does nothing
        assert alone(ctx.handle, M, None, 0, None, None, 0, N, None, 1, 1.5, None, None, None) == 0
        assert both(ctx.handle, M, None, 0, None, None, 0, N, None, None, None, None, None, None, None, 1, 1.5, None, None, None, None) == 0
        assert untouched()
    from tft_vs_fund_amd import api                                          # the wrapper judges before it calls
    with pytest.raises(ValueError):
        ctx.bundle_adjust_views(CalM, R_t[None], Cp[None], None, missing="view", cov=True)


def test_predicted_covariance_is_the_scatter_of_the_result():
    """M = 4, N = 64, the `random` pattern, no loss: 2 048 draws of 1 px noise as ONE batch started at the truth, cov=True.  The empirical over the
    predicted standard deviation of every estimated camera parameter is within 0.08 of 1: the relative standard error of a sample deviation over T
    draws is 1 / sqrt(2 (T - 1)) = 0.0156, and 0.08 is five of those (the bound of tests/test_gpu_ba_cov.py for the three-view statistic)."""
    ms = tcc.mc_scene()
    Cs = tcc.mc_draws()
    T = Cs.shape[0]
    assert T == 2048 and abs(1.0 / np.sqrt(2.0 * (T - 1)) - 0.0156) < 1e-4
    out = _ctx().bundle_adjust_views(ms["CalM"], np.broadcast_to(ms["R_t"], (T,) + ms["R_t"].shape).copy(), Cs, np.broadcast_to(ms["X"], (T, 3, tcc.MC_N)).copy(),
                                     missing="point", cov=True)
    torch.cuda.synchronize()
    assert int((out["status"] != 0).sum()) == 0 and int((out["used"] != tcc.MC_N).sum()) == 0
    cov = out["cov"].cpu().numpy()
    assert np.isfinite(cov).all()
    ratio = tcc.mc_ratio(tcc.mc_params(out["R_t"].cpu().numpy()), cov)
    print("empirical / predicted standard deviation:", np.round(ratio, 3))
    assert ratio.shape == (6 * (tcc.MC_M - 1),) and np.abs(ratio - 1.0).max() <= tcc.MC_BOUND, ratio
