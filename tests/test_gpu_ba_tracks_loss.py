"""
The bundle adjustment over tracks with a robust loss on the GPU (tff_bundle_adjust_tracks_loss_batch_dev / _host, include/tftfund_tracks_loss.h;
Context.bundle_adjust_views and api.BundleAdjustment with missing="point", loss=, scale=) against the numpy restatement
(tests/ba_tracks_loss_oracle.py) over the cases of tests/ba_tracks_loss_cases.py at its gate.  All cases of one (M, loss, scale, Reconst0 or not) go into
ONE call, NaN-padded to N = 130: the padding contract is thereby tested on every case.  Bit for bit: an item alone and inside the padded batch, N = 65
padded to 130, _host and _dev, loss=None and the plain tracks call.  The failing items, every TFF_E_INVALID, and what the loss is for.
"""
import ctypes
import functools

import numpy as np
import pytest

import ba_tracks_cases as tc
import ba_tracks_loss_cases as lc
import ba_tracks_oracle as TO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
LOSS_ID = {None: 0, "huber": 1, "cauchy": 2}
NPAD = 130
E_INVALID = -10001


@functools.lru_cache(maxsize=None)
def _ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    return api.Context(0)


def _padded(case, n):
    CalM, R0, C, X0 = case[:4]
    k = n - C.shape[1]
    return (CalM, R0, np.hstack([C, np.full((C.shape[0], k), np.nan)]), None if X0 is None else np.hstack([X0, np.full((3, k), 7.0)]))


def _cut(o, b, n):
    """item b of the batch's outputs, its first n columns"""
    return dict(R_t=o["R_t"][b], Reconst=o["Reconst"][b][:, :n], iter=int(o["iter"][b]), repr_err=float(o["repr_err"][b]), used=int(o["used"][b]),
                status=int(o["status"][b]), weight=o["weight"][b][:n], tail=(o["Reconst"][b][:, n:], o["weight"][b][n:]))


def _dev(cases, loss, scale, pad=None):
    """cases: [(CalM, R0, C, X0)] of one M, all with or all without X0, padded to `pad` columns -> per item the dict of lc.gate"""
    ns = [c[2].shape[1] for c in cases]
    pad = max(ns) if pad is None else pad
    cs = [_padded(c, pad) for c in cases]
    X0 = np.stack([c[3] for c in cs]) if cs[0][3] is not None else None
    out = _ctx().bundle_adjust_views(cs[0][0], np.stack([c[1] for c in cs]), np.stack([np.ascontiguousarray(c[2].T) for c in cs]), X0, missing="point", loss=loss, scale=scale)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    if loss is None:
        o["weight"] = np.full((len(cs), pad, cs[0][2].shape[0] // 2), np.nan)            # (the plain call has none)
    return [_cut(o, b, n) for b, n in enumerate(ns)]


def _host(cases, loss, scale, pad=None, weight=True):
    ctx = _ctx()
    ns = [c[2].shape[1] for c in cases]
    N = max(ns) if pad is None else pad
    cs = [_padded(c, N) for c in cases]
    B = len(cs); M = cs[0][2].shape[0] // 2
    calm = np.ascontiguousarray(cs[0][0].T).reshape(-1)
    rt = np.stack([np.ascontiguousarray(c[1].T).reshape(-1) for c in cs]); Cc = np.stack([np.ascontiguousarray(c[2].T) for c in cs])
    x0 = np.stack([np.ascontiguousarray(c[3].T) for c in cs]) if cs[0][3] is not None else None
    o = np.full((B, 12 * M), 5.0); rec = np.full((B, N, 3), 5.0); it = np.full(B, 5, dtype=np.int32); err = np.full(B, 5.0)
    used = np.full(B, -5, dtype=np.int32); st = np.full(B, 5, dtype=np.int32); w = np.full((B, N, M), 5.0)
    assert ctx.lib.tff_bundle_adjust_tracks_loss_batch_host(ctx.handle, M, P(calm), 0, P(rt), P(Cc), B, N, P(x0), P(o), P(rec), P(it), P(err), P(used), P(st),
                                                            LOSS_ID[loss], 0.0 if scale is None else float(scale), P(w) if weight else None) == 0
    out = dict(R_t=np.stack([o[b].reshape(4, 3 * M).T for b in range(B)]), Reconst=rec.transpose(0, 2, 1), iter=it, repr_err=err, used=used, status=st, weight=w)
    return [_cut(out, b, n) for b, n in enumerate(ns)]


def _biteq(a, b, tail=True):
    keys = ("R_t", "Reconst", "weight")
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in keys) \
        and (a["iter"], a["used"], a["status"]) == (b["iter"], b["used"], b["status"]) and np.array([a["repr_err"]]).tobytes() == np.array([b["repr_err"]]).tobytes()


def _group(M, loss, c, with_x0):
    twin = (loss, c) == lc.TWIN
    pats = lc.TWIN_PATTERNS if twin else lc.PATTERNS
    return [(M, N, p, loss, c) for N in lc.SIZES if (N % 2 == 0) == with_x0 for p in pats if tc.applicable(M, N, p)]


GROUPS = [(M, loss, c, x0) for M in lc.VIEWS for loss, c in lc.LOSSES + (lc.TWIN,) for x0 in (False, True)]


def test_the_groups_cover_every_case():
    assert sorted(k for g in GROUPS for k in _group(*g)) == sorted(lc.CASES)


@pytest.mark.parametrize("M,loss,c,with_x0", GROUPS)
def test_every_case_matches_the_restatement_dev_and_host(M, loss, c, with_x0):
    keys = _group(M, loss, c, with_x0)
    cases = [lc.inputs(*k[:3]) for k in keys]
    dev, host = _dev(cases, loss, c, NPAD), _host(cases, loss, c, NPAD)
    for k, d, h in zip(keys, dev, host):
        ref = lc.restated(*k)
        print(k, "iter", d["iter"], ref["iter"], "repr_err", d["repr_err"], ref["repr_err"], "compared", k not in lc.LEFT_OUT)
        assert (k not in lc.LEFT_OUT) == lc.compared(ref), k
        lc.gate(d, ref, k + ("dev",), full=k not in lc.LEFT_OUT)
        lc.gate(h, ref, k + ("host",), full=k not in lc.LEFT_OUT)
        assert _biteq(d, h), k                                               # the same kernel on the same bytes
        for t in (d, h):                                                     # the padding: NaN, and nothing else
            assert np.isnan(t["tail"][0]).all() and np.isnan(t["tail"][1]).all(), k


@pytest.mark.parametrize("M,N", [(3, 65), (6, 130)])
@pytest.mark.parametrize("loss,c", lc.LOSSES)
def test_an_item_alone_equals_the_item_in_the_padded_batch(M, N, loss, c):
    """one wavefront per problem and inert NaN columns: the item at its own N and B = 1, against the same item padded to 130 among the other cases"""
    with_x0 = N % 2 == 0
    keys = _group(M, loss, c, with_x0)
    batch = _dev([lc.inputs(*k[:3]) for k in keys], loss, c, NPAD)
    k = (M, N, "random", loss, c)
    alone = _dev([lc.inputs(M, N, "random")], loss, c)[0]
    assert alone["weight"].shape == (N, M) and _biteq(alone, batch[keys.index(k)]), k
    host = _host([lc.inputs(M, N, "random")], loss, c)[0]
    assert _biteq(alone, host), k
    no_w = _host([lc.inputs(M, N, "random")], loss, c, weight=False)[0]       # weight may be NULL
    assert no_w["R_t"].tobytes() == alone["R_t"].tobytes() and no_w["iter"] == alone["iter"]


@pytest.mark.parametrize("M,N", [(3, 65), (6, 130)])
def test_loss_none_is_the_plain_tracks_call(M, N):
    ctx = _ctx()
    case = lc.inputs(M, N, "random")
    plain = _dev([case], None, None)[0]                                      # tff_bundle_adjust_tracks_batch_dev
    for scale in (None, float("nan")):                                       # scale is not read
        got = _host([case], None, scale)[0]
        vis = TO.visibility(case[2])
        want = np.where(vis & (vis.sum(axis=0) >= 2)[None], 1.0, np.nan).T
        assert np.array_equal(got["weight"], want, equal_nan=True) and (want == 1.0).any() and np.isnan(want).any()
        got["weight"] = plain["weight"]
        assert _biteq(got, plain), (M, N)
    # ... and through _dev, on device buffers of the caller
    Cc = torch.from_numpy(np.ascontiguousarray(case[2].T)[None]).cuda(); calm = torch.from_numpy(np.ascontiguousarray(case[0].T).reshape(-1)).cuda()
    rt = torch.from_numpy(np.ascontiguousarray(case[1].T).reshape(1, -1)).cuda()
    x0 = torch.from_numpy(np.ascontiguousarray(case[3].T)[None]).cuda() if case[3] is not None else None
    o = torch.empty((1, 12 * M), dtype=torch.float64, device="cuda"); rec = torch.empty((1, N, 3), dtype=torch.float64, device="cuda")
    w = torch.empty((1, N, M), dtype=torch.float64, device="cuda"); err = torch.empty(1, dtype=torch.float64, device="cuda")
    it = torch.zeros(1, dtype=torch.int32, device="cuda"); used = torch.zeros_like(it)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    assert ctx.lib.tff_bundle_adjust_tracks_loss_batch_dev(ctx.handle, M, p(calm), 0, p(rt), p(Cc), 1, N, p(x0), p(o), p(rec), p(it), p(err), p(used), None, 0, 0.0, p(w)) == 0
    torch.cuda.synchronize()                                                 # (no status output: the weights still know which item failed)
    assert np.array_equal(w.cpu().numpy()[0], want, equal_nan=True)
    assert o.cpu().numpy()[0].reshape(4, 3 * M).T.tobytes() == np.ascontiguousarray(plain["R_t"]).tobytes() and int(it[0]) == plain["iter"]


@pytest.mark.parametrize("loss,c", lc.LOSSES + ((None, None),))
def test_failing_items_inside_a_batch_of_good_ones(loss, c):
    for kind in tc.FAILING:
        case, used, status = tc.failing(kind)
        with_x0 = case[3] is not None
        good = [tc.synthetic(3, 12, "random", with_x0), tc.synthetic(3, 12, "full", with_x0)]
        batch = [good[0], case, good[1]]
        for run in (_dev, _host):
            if run is _dev and loss is None:
                continue                                                     # (that is the plain call: tests/test_gpu_ba_tracks.py)
            got = run(batch, loss, c)
            assert (got[1]["used"], got[1]["status"]) == (used, status), (kind, run.__name__)
            lc.gate(got[1], lc.restated_failing(kind, loss, c), (kind, loss, run.__name__))
            for b, g in ((0, good[0]), (2, good[1])):                         # the neighbours are what they are alone
                assert got[b]["status"] == 0 and _biteq(got[b], run([g], loss, c)[0]), (kind, b)
    from tft_vs_fund_amd import api
    if loss is not None:
        with pytest.raises(ValueError):
            api.BundleAdjustment(*tc.failing("too_few")[0], missing="point", loss=loss, scale=c)


def test_every_invalid_argument_is_refused_before_any_work():
    ctx = _ctx()
    M, N, B = 3, 12, 1
    CalM, R0, C, X0 = tc.synthetic(M, N, "full", False)
    calm = np.ascontiguousarray(CalM.T).reshape(-1); rt = np.ascontiguousarray(R0.T).reshape(-1); Cc = np.ascontiguousarray(C.T)
    o = np.full(12 * M, 5.0)
    good = dict(M=M, calm=P(calm), stride=0, rt=P(rt), C=P(Cc), B=B, N=N, out=P(o), loss=1, scale=1.5)
    bad = [dict(loss=3), dict(loss=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(loss=2, scale=0.0),
           dict(M=1), dict(M=7), dict(B=-1), dict(N=-1), dict(N=0), dict(calm=None), dict(rt=None), dict(C=None), dict(out=None), dict(stride=5),
           dict(loss=0, M=7), dict(loss=0, calm=None)]
    for fn in (ctx.lib.tff_bundle_adjust_tracks_loss_batch_host, ctx.lib.tff_bundle_adjust_tracks_loss_batch_dev):
        for ch in bad:
            a = dict(good); a.update(ch)
            r = fn(ctx.handle, a["M"], a["calm"], a["stride"], a["rt"], a["C"], a["B"], a["N"], None, a["out"], None, None, None, None, None, a["loss"], a["scale"], None)
            assert r == E_INVALID and len(ctx.lib.tff_last_error()) > 0, (fn.__name__, ch)
            assert o.tobytes() == np.full(12 * M, 5.0).tobytes()
        assert fn(None, M, good["calm"], 0, good["rt"], good["C"], B, N, None, good["out"], None, None, None, None, None, 1, 1.5, None) == E_INVALID
        assert ctx.lib.tff_last_error().decode() == "null context"
    # with TFF_LOSS_NONE the scale is not read, and B = 0 is a call that does nothing
    assert ctx.lib.tff_bundle_adjust_tracks_loss_batch_host(ctx.handle, M, P(calm), 0, P(rt), P(Cc), B, N, None, P(o), None, None, None, None, None, 0, float("nan"), None) == 0
    assert ctx.lib.tff_bundle_adjust_tracks_loss_batch_host(ctx.handle, M, None, 0, None, None, 0, N, None, None, None, None, None, None, None, 1, 1.5, None) == 0


@pytest.mark.parametrize("n", lc.PURPOSE_SIZES)
def test_what_the_loss_is_for(n):
    """three views, 5 % of the single observations displaced by 20 .. 80 px: under Cauchy at 3 px the worst rotation error is below half of that of the
    plain run (the restatement shows a factor of 14 and more), and every displaced observation gets a weight below 0.1"""
    CalM, R0, C, X0, truth, bad = lc.purpose_scene(n)
    plain = _dev([(CalM, R0, C, X0)], None, None)[0]
    robust = _dev([(CalM, R0, C, X0)], "cauchy", 3.0)[0]
    assert plain["status"] == 0 and robust["status"] == 0
    e0, e1 = lc.worst_rot_err_deg(plain["R_t"], truth), lc.worst_rot_err_deg(robust["R_t"], truth)
    wbad = np.array([robust["weight"][i, v] for v, i in bad])
    print("n", n, "worst rotation error, degrees: plain", e0, "cauchy", e1, "largest weight of a displaced observation", wbad.max())
    assert e1 < 0.5 * e0, (e0, e1)
    assert (wbad < 0.1).all(), wbad
    from tft_vs_fund_amd import api
    R_t, Rec, it, err = api.BundleAdjustment(CalM, R0, C, X0, missing="point", loss="cauchy", scale=3.0)
    assert it == robust["iter"] and R_t.tobytes() == np.ascontiguousarray(robust["R_t"]).tobytes() and err == robust["repr_err"]
