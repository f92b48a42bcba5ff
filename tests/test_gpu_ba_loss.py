"""
Robust losses in the three-view bundle adjustment on the GPU (tff_bundle_adjust_loss_*, Context.bundle_adjust(..., loss=),
Context.bundle_adjust_ragged(..., loss=), the polish_* arguments of the robust estimators; include/tftfund_loss.h).

  1. the three kernel instances against the numpy restatement (tests/ba_loss_oracle.py): the cases and the gate of tests/test_emulated_ba_loss.py;
  2. the ragged call against the fixed-N loss call, bit for bit, weights included;
  3. no loss through the new entry points against the existing ones, bit for bit;
  4. the robust calls with a loss in the polish: a scene in a list = the scene alone = bundle_adjust_ragged by hand;
  5. end to end on the scene of 100 matches with 30 displaced, whose condition tests/test_ba_loss_cpu.py asserts on the restatement.

"""
import ctypes
import functools
import os

import numpy as np
import pytest

import ba_loss_cases as bc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@functools.lru_cache(maxsize=None)
def _ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    ctx = api.Context(0)
    ctx.set_ba_classes(2)                                                     # three launch classes unless a test says otherwise
    return ctx


def _bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _np(out):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def _fixed(C, CalM, start, X0, loss, c):
    """Context.bundle_adjust with B = 1: C (n, 6), X0 (n, 3) or None"""
    return _np(_ctx().bundle_adjust(CalM, start[0][None], start[1][None], np.ascontiguousarray(C)[None], None if X0 is None else np.ascontiguousarray(X0.T)[None],
                                    loss=loss, scale=c))


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_bad,loss,c,with_x0", bc.CASES)
def test_loss_instances_match_the_restatement(n, n_bad, loss, c, with_x0):
    sc = bc.scene(n, n_bad)
    ref = bc.restated(n, n_bad, loss, c, with_x0)
    o = _fixed(sc["C"], sc["CalM"], sc["start"], sc["X0"] if with_x0 else None, loss, c)
    assert o["weight"].shape == (1, n)
    bc.gate(ref, int(o["status"][0]), int(o["iter"][0]), float(o["repr_err"][0]), o["R_t_2"][0], o["R_t_3"][0], o["Reconst"][0], o["weight"][0],
            (n, n_bad, loss, c, with_x0))


# ---- 2. ragged equals fixed-N ---------------------------------------------------------------------------------------------------------------------------
def _exact_mask(n, keep, rng):
    row = np.zeros(n, dtype=np.uint8)
    row[rng.choice(n, keep, replace=False)] = rng.choice([1, 255], keep)
    return row


@functools.lru_cache(maxsize=None)
def _items(sizes):
    """a scene per size (a tenth of its matches displaced), each with its own focal length and so its own CalM; a scene of 0 matches is empty arrays"""
    out = []
    for k, n in enumerate(sizes):
        sc = bc.scene(max(n, 12), max(n, 12) // 10, seed=300 + k, focalL=38.0 + 3.0 * k)
        out.append(dict(C=sc["C"][:n], CalM=sc["CalM"], start=sc["start"], X0=sc["X0"][:n]))
    return out


@pytest.mark.parametrize("with_x0", (False, True))
@pytest.mark.parametrize("mask_kind", ("none", "random", "ones"))
@pytest.mark.parametrize("loss,c", (("huber", 3.0), ("cauchy", 3.0)))
def test_ragged_items_equal_the_fixed_loss_call(loss, c, mask_kind, with_x0):
    from tft_vs_fund_amd import api
    ctx = _ctx()
    b0 = int(api.ba_ragged_class_bounds()[0])
    counts = (b0 + 1, 0, 1, 12, 40, 64, 65, 129, b0)                          # permuted: item 0 is of the second class
    sizes = tuple(int(np.ceil(m / 0.7)) if mask_kind == "random" and m else m for m in counts)
    items = _items(sizes)
    rng = np.random.default_rng(11)
    masks = None if mask_kind == "none" else [_exact_mask(n, m, rng) if mask_kind == "random" else np.ones(n, dtype=np.uint8) for n, m in zip(sizes, counts)]
    sels = [np.ones(n, dtype=bool) if masks is None else masks[k] != 0 for k, n in enumerate(sizes)]
    packed, off = api.pack_ragged([it["C"] for it in items])
    calm = np.stack([it["CalM"] for it in items])
    s2 = np.stack([it["start"][0] for it in items]); s3 = np.stack([it["start"][1] for it in items])
    x0 = np.concatenate([it["X0"] for it in items]) if with_x0 else None
    mask = None if masks is None else np.concatenate(masks)
    cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dev = _np(ctx.bundle_adjust_ragged(cu(calm), cu(s2), cu(s3), cu(packed), cu(off), mask=cu(mask), reconst0=cu(x0), loss=loss, scale=c))
    host = ctx.bundle_adjust_ragged(calm, s2, s3, packed, off, mask=mask, reconst0=x0, loss=loss, scale=c)
    for k in ("R_t_2", "R_t_3", "Reconst", "repr_err", "weight"):              # the host form equals the device form
        assert np.array_equal(_bits(host[k]), _bits(dev[k])), k
    for k in ("iter", "status", "used"):
        assert np.array_equal(host[k], dev[k]), k
    some_down = False
    for b, it in enumerate(items):
        o0, o1 = int(off[b]), int(off[b + 1])
        sel, m = sels[b], int(sels[b].sum())
        if m == 0:
            assert dev["status"][b] == api.ST_TOO_FEW and np.isnan(dev["R_t_2"][b]).all() and np.isnan(dev["weight"][o0:o1]).all(), b
            continue
        ref = _fixed(it["C"][sel], it["CalM"], it["start"], it["X0"][sel] if with_x0 else None, loss, c)
        assert int(dev["status"][b]) == int(ref["status"][0]) and int(dev["iter"][b]) == int(ref["iter"][0]) and int(dev["used"][b]) == m, b
        assert (int(ref["status"][0]) == 0) == (m > 1), b
        for k in ("R_t_2", "R_t_3", "repr_err"):
            assert np.array_equal(_bits(dev[k][b]), _bits(ref[k][0])), (b, k)
        assert np.array_equal(_bits(dev["Reconst"][o0:o1][sel]), _bits(ref["Reconst"][0].T)) and np.isnan(dev["Reconst"][o0:o1][~sel]).all(), b
        assert np.array_equal(_bits(dev["weight"][o0:o1][sel]), _bits(ref["weight"][0])) and np.isnan(dev["weight"][o0:o1][~sel]).all(), b
        if m > 1:
            w = ref["weight"][0]
            assert (w > 0).all() and (w <= 1).all()
            some_down |= bool((w < 0.5).any())
    assert some_down
    if mask_kind == "none" and not with_x0:                                   # a decreasing offset leaves its neighbours' bits alone
        bad = off.copy(); bad[5] = bad[4] - 3                                 # item 4 ends before it starts; item 5 starts inside item 3's range
        out = _np(ctx.bundle_adjust_ragged(cu(calm), cu(s2), cu(s3), cu(packed), cu(bad), loss=loss, scale=c))
        assert out["status"][4] == api.ST_BAD_OFFSETS and np.isnan(out["R_t_2"][4]).all()
        for b in (0, 2, 6, 7, 8):
            o0, o1 = int(off[b]), int(off[b + 1])
            assert out["status"][b] == dev["status"][b] and out["iter"][b] == dev["iter"][b], b
            for k in ("R_t_2", "R_t_3", "repr_err"):
                assert np.array_equal(_bits(out[k][b]), _bits(dev[k][b])), (b, k)
            assert np.array_equal(_bits(out["weight"][o0:o1]), _bits(dev["weight"][o0:o1])), b


# ---- 3. no loss -------------------------------------------------------------------------------------------------------------------------------------------
def test_no_loss_is_the_existing_call_bit_for_bit():
    """loss=None takes the existing entry points; TFF_LOSS_NONE through the new ones gives their bits, whatever the scale, and weights of 1"""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    lib = ctx.lib
    sizes = (40, 12, 129, 0, 65)
    items = _items(sizes)
    packed, off = api.pack_ragged([it["C"] for it in items])
    nt, B = packed.shape[0], len(sizes)
    calm = np.stack([it["CalM"] for it in items])
    s2 = np.stack([it["start"][0] for it in items]); s3 = np.stack([it["start"][1] for it in items])
    rng = np.random.default_rng(2)
    mask = (rng.random(nt) < 0.8).astype(np.uint8)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    for mk in (None, mask):
        old = ctx.bundle_adjust_ragged(calm, s2, s3, packed, off, mask=mk)
        assert "weight" not in old
        calm_cm = np.ascontiguousarray(calm.transpose(0, 2, 1)).reshape(-1)
        r2 = np.ascontiguousarray(s2.transpose(0, 2, 1)); r3 = np.ascontiguousarray(s3.transpose(0, 2, 1))
        o2 = np.empty((B, 12)); o3 = np.empty((B, 12)); rec = np.full((nt, 3), np.nan); it = np.zeros(B, dtype=np.int32); st = np.zeros(B, dtype=np.int32)
        used = np.zeros(B, dtype=np.int32); err = np.empty(B); w = np.full(nt, 7.0)
        rc = lib.tff_bundle_adjust_loss_ragged_host(ctx.handle, P(packed), P(off), P(mk), P(calm_cm), 27, P(r2), P(r3), None, B, P(o2), P(o3), P(rec), P(it), P(err),
                                                    P(used), P(st), 0, float("nan"), P(w))
        assert rc == 0
        assert np.array_equal(_bits(o2.reshape(B, 4, 3).transpose(0, 2, 1)), _bits(old["R_t_2"])) and np.array_equal(_bits(o3.reshape(B, 4, 3).transpose(0, 2, 1)), _bits(old["R_t_3"]))
        assert np.array_equal(_bits(rec), _bits(old["Reconst"])) and np.array_equal(_bits(err), _bits(old["repr_err"]))
        assert np.array_equal(it, old["iter"]) and np.array_equal(st, old["status"]) and np.array_equal(used, old["used"])
        sel = np.ones(nt, dtype=bool) if mk is None else mk != 0
        assert (w[sel] == 1.0).all() and np.isnan(w[~sel]).all()
        assert lib.tff_bundle_adjust_loss_ragged_host(ctx.handle, P(packed), P(off), P(mk), P(calm_cm), 27, P(r2), P(r3), None, B, P(o2), P(o3), P(rec), P(it), P(err),
                                                      P(used), P(st), 3, 1.0, P(w)) == -10001
        assert lib.tff_bundle_adjust_loss_ragged_host(ctx.handle, P(packed), P(off), P(mk), P(calm_cm), 27, P(r2), P(r3), None, B, P(o2), P(o3), P(rec), P(it), P(err),
                                                      P(used), P(st), 1, 0.0, P(w)) == -10001
    # fixed N, the device form
    it0 = items[0]
    old = _fixed(it0["C"], it0["CalM"], it0["start"], None, None, None)
    assert "weight" not in old
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    C = cu(it0["C"][None]); cm = cu(it0["CalM"].T.reshape(27)); r2 = cu(it0["start"][0].T.reshape(1, 12)); r3 = cu(it0["start"][1].T.reshape(1, 12))
    n = it0["C"].shape[0]
    o2 = torch.empty((1, 12), dtype=torch.float64, device="cuda"); o3 = torch.empty_like(o2); rec = torch.empty((1, n, 3), dtype=torch.float64, device="cuda")
    it = torch.zeros(1, dtype=torch.int32, device="cuda"); st = torch.zeros_like(it); err = torch.empty(1, dtype=torch.float64, device="cuda")
    w = torch.full((1, n), 7.0, dtype=torch.float64, device="cuda")
    p = ctx._p
    assert lib.tff_bundle_adjust_loss_batch_dev(ctx.handle, p(cm), 0, p(r2), p(r3), p(C), 1, n, None, p(o2), p(o3), p(rec), p(it), p(err), p(st), 0, -5.0, p(w)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(o2.reshape(1, 4, 3).transpose(1, 2)), _bits(old["R_t_2"])) and np.array_equal(_bits(o3.reshape(1, 4, 3).transpose(1, 2)), _bits(old["R_t_3"]))
    assert np.array_equal(_bits(rec.transpose(1, 2)), _bits(old["Reconst"])) and np.array_equal(_bits(err), _bits(old["repr_err"]))
    assert int(it[0]) == int(old["iter"][0]) and int(st[0]) == 0 and bool((w == 1.0).all())


def _batch_host(ctx, items, loss_id, scale, with_weight=True, with_x0=False):
    """tff_bundle_adjust_loss_batch_host on B items of one size, host pointers"""
    B, n = len(items), items[0]["C"].shape[0]
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    C = np.ascontiguousarray(np.stack([it["C"] for it in items]))
    calm = np.ascontiguousarray(np.stack([it["CalM"].T.reshape(27) for it in items]))
    r2 = np.ascontiguousarray(np.stack([it["start"][0].T.reshape(12) for it in items])); r3 = np.ascontiguousarray(np.stack([it["start"][1].T.reshape(12) for it in items]))
    x0 = np.ascontiguousarray(np.stack([it["X0"] for it in items])) if with_x0 else None
    o = dict(o2=np.empty((B, 12)), o3=np.empty((B, 12)), rec=np.empty((B, n, 3)), iter=np.zeros(B, dtype=np.int32), err=np.empty(B), st=np.full(B, -7, dtype=np.int32),
             w=np.full((B, n), 7.0) if with_weight else None)
    rc = ctx.lib.tff_bundle_adjust_loss_batch_host(ctx.handle, P(calm), 27, P(r2), P(r3), P(C), B, n, P(x0), P(o["o2"]), P(o["o3"]), P(o["rec"]), P(o["iter"]), P(o["err"]),
                                                   P(o["st"]), loss_id, scale, P(o["w"]))
    assert rc == 0
    return dict(R_t_2=o["o2"].reshape(B, 4, 3).transpose(0, 2, 1), R_t_3=o["o3"].reshape(B, 4, 3).transpose(0, 2, 1), Reconst=o["rec"].transpose(0, 2, 1), iter=o["iter"],
                repr_err=o["err"], status=o["st"], weight=o["w"])


@pytest.mark.parametrize("with_x0", (False, True))
@pytest.mark.parametrize("loss,c", (("huber", 3.0), ("cauchy", 1.5), (None, None)))
def test_batch_host_equals_the_device_form(loss, c, with_x0):
    """three items of 65 matches, a CalM each: the host form of the fixed-N loss call, with its staged weights, gives the bits of the device form;
    without a weight output nothing else changes; TFF_LOSS_NONE gives the bits of the existing calls and weights of 1"""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    items = _items((65, 65, 65))
    B = len(items)
    calm = np.stack([it["CalM"] for it in items]); s2 = np.stack([it["start"][0] for it in items]); s3 = np.stack([it["start"][1] for it in items])
    C = np.stack([it["C"] for it in items]); x0 = np.stack([it["X0"].T for it in items]) if with_x0 else None
    dev = _np(ctx.bundle_adjust(calm, s2, s3, C, x0, loss=loss, scale=c))     # tff_bundle_adjust_batch_dev / tff_bundle_adjust_loss_batch_dev
    host = _batch_host(ctx, items, api.LOSS_IDS.get(loss, 0), c if c else float("nan"), with_x0=with_x0)
    assert (loss is None or (dev["status"] == 0).all()) and np.array_equal(host["status"], dev["status"]) and np.array_equal(host["iter"], dev["iter"])
    for k in ("R_t_2", "R_t_3", "Reconst", "repr_err"):
        assert np.array_equal(_bits(host[k]), _bits(dev[k])), k
    if loss is None:
        assert "weight" not in dev and (host["weight"] == 1.0).all()
    else:
        assert np.array_equal(_bits(host["weight"]), _bits(dev["weight"])) and (host["weight"] > 0).all() and host["weight"].min() < 0.5
    bare = _batch_host(ctx, items, api.LOSS_IDS.get(loss, 0), c if c else 0.0, with_weight=False, with_x0=with_x0)
    for k in ("R_t_2", "R_t_3", "Reconst", "repr_err"):
        assert np.array_equal(_bits(bare[k]), _bits(host[k])), k
    assert np.array_equal(bare["iter"], host["iter"])
    # the same items through the ragged device form with TFF_LOSS_NONE / the loss: the bits of the fixed-N device form
    packed, off = api.pack_ragged([it["C"] for it in items])
    cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xr = cu(np.concatenate([it["X0"] for it in items])) if with_x0 else None
    if loss is None:
        p = ctx._p
        t = dict(c=cu(np.stack([it["CalM"].T.reshape(27) for it in items]).reshape(-1)), r2=cu(np.stack([it["start"][0].T.reshape(12) for it in items])),
                 r3=cu(np.stack([it["start"][1].T.reshape(12) for it in items])), pk=cu(packed), off=cu(off))
        nt = packed.shape[0]
        o2 = torch.empty((B, 12), dtype=torch.float64, device="cuda"); o3 = torch.empty_like(o2); rec = torch.empty((nt, 3), dtype=torch.float64, device="cuda")
        it_ = torch.zeros(B, dtype=torch.int32, device="cuda"); st = torch.zeros_like(it_); used = torch.zeros_like(it_); err = torch.empty(B, dtype=torch.float64, device="cuda")
        w = torch.full((nt,), 7.0, dtype=torch.float64, device="cuda")
        assert ctx.lib.tff_bundle_adjust_loss_ragged_dev(ctx.handle, p(t["pk"]), p(t["off"]), nt, None, p(t["c"]), 27, p(t["r2"]), p(t["r3"]), p(xr), B, p(o2), p(o3), p(rec),
                                                         p(it_), p(err), p(used), p(st), 0, float("inf"), p(w)) == 0
        torch.cuda.synchronize()
        rag = dict(R_t_2=o2.reshape(B, 4, 3).transpose(1, 2), R_t_3=o3.reshape(B, 4, 3).transpose(1, 2), repr_err=err, iter=it_.cpu().numpy())
        assert bool((w == 1.0).all())
        recs = rec.cpu().numpy()
    else:
        rag = _np(ctx.bundle_adjust_ragged(cu(calm), cu(s2), cu(s3), cu(packed), cu(off), reconst0=xr, loss=loss, scale=c))
        assert np.array_equal(_bits(rag["weight"]), _bits(dev["weight"].reshape(-1)))
        recs = rag["Reconst"]
    for k in ("R_t_2", "R_t_3", "repr_err"):
        assert np.array_equal(_bits(rag[k]), _bits(dev[k])), k
    assert np.array_equal(np.asarray(rag["iter"]), dev["iter"]) and np.array_equal(_bits(recs.reshape(B, 65, 3).transpose(0, 2, 1)), _bits(dev["Reconst"]))


# ---- 4. the robust calls -----------------------------------------------------------------------------------------------------------------------------------
def _synthetic(n, gen_seed):
    """the recipe of tests/test_gpu_robust_scenes.py: 0.5 px noise, a quarter of the matches displaced by U(20, 80) px in views 2, 3"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, n, noise=0.5, seed=gen_seed)
    scene = C[0].copy()
    rng = np.random.default_rng(gen_seed + 100)
    bad = rng.choice(n, n // 4, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    return np.ascontiguousarray(scene), np.ascontiguousarray(CalM)


def _fountain(t):
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epfl_all.npz"))
    off, K, trip = d["fountain_offsets"], d["fountain_K"], d["fountain_triplets"]
    return np.ascontiguousarray(d["fountain_corresp"][off[t]:off[t + 1]]), np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0)


@pytest.mark.parametrize("polish_all", (False, True))
def test_robust_calls_with_a_loss_in_the_polish(polish_all):
    """five scenes like those of test_scenes_refine: 5 (no pose), 61, 150, 400 synthetic matches and one fountain triplet"""
    from tft_vs_fund_amd import api
    ctx = _ctx()
    method, n_hyp, thr, seed = "LinearTFTPoseEstimation", 300, 4.0, 21
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epfl_all.npz"))
    t = int(np.nonzero((np.diff(d["fountain_offsets"]) > 300) & (np.diff(d["fountain_offsets"]) < 900))[0][0])
    pairs = [_synthetic(n, 40 + k) for k, n in enumerate((5, 61, 150, 400))] + [_fountain(t)]
    packed, off = api.pack_ragged([a for a, _ in pairs])
    calms = np.stack([c for _, c in pairs])
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kw = dict(polish=True, polish_loss="cauchy", polish_all=polish_all)       # polish_scale: the threshold
    out = _np(ctx.robust_pose_scenes(method, cu(packed), cu(off), cu(calms), n_hyp, thr, seed=seed, ns_max=int(np.diff(off).max()), **kw))
    keys = ("R_t_2_polished", "R_t_3_polished", "repr_err_polished", "weight_polished")
    assert out["weight_polished"].shape == out["mask"].shape
    # by hand on the result's poses and mask
    hand = _np(ctx.bundle_adjust_ragged(cu(calms), cu(out["R_t_2"]), cu(out["R_t_3"]), cu(packed), cu(off), mask=None if polish_all else cu(out["mask"]),
                                        reconst=False, loss="cauchy", scale=thr))
    for k in keys:
        assert np.array_equal(_bits(out[k]), _bits(hand[k[:-9]])), k
    assert np.array_equal(out["iter_polished"], hand["iter"]) and np.array_equal(out["status_polished"], hand["status"])
    # the numpy form, and scene by scene robust_pose with seed + s
    host = ctx.robust_pose_scenes(method, packed, off, calms, n_hyp, thr, seed=seed, **kw)
    for k in keys:
        assert np.array_equal(_bits(host[k]), _bits(out[k])), k
    for s, (scene, calm) in enumerate(pairs):
        o0, o1 = int(off[s]), int(off[s + 1])
        if scene.shape[0] < api.ROBUST_METHODS[method]:                       # (the one-scene call refuses a scene smaller than a sample)
            continue
        one = _np(ctx.robust_pose(method, cu(scene), cu(calm), n_hyp, thr, seed=seed + s, **kw))
        for k in keys[:3]:
            assert np.array_equal(_bits(one[k]), _bits(out[k][s])), (s, k)
        assert np.array_equal(_bits(one["weight_polished"]), _bits(out["weight_polished"][o0:o1])), s
        assert int(one["iter_polished"]) == int(out["iter_polished"][s]) and int(one["status_polished"]) == int(out["status_polished"][s]), s
    # a scene without a pose: nothing selected under the mask (ST_TOO_FEW); over all matches its NaN poses enter the adjustment (ST_NONFINITE)
    assert out["status"][0] != 0 and out["status_polished"][0] == (api.ST_NONFINITE if polish_all else api.ST_TOO_FEW)
    assert np.isnan(out["weight_polished"][:5]).all() and np.isnan(out["R_t_2_polished"][0]).all()
    ok = out["status"] == 0
    assert ok[1:].all() and (out["status_polished"][1:] == 0).all()
    w, m = out["weight_polished"][5:], out["mask"][5:] != 0
    if polish_all:
        assert not np.isnan(w).any() and np.median(w[m]) > np.median(w[~m])           # the weight falls with the residual: the hard rule's outliers are kept down
    else:
        assert np.isnan(w[~m]).all() and not np.isnan(w[m]).any()
    without = _np(ctx.robust_pose_scenes(method, cu(packed), cu(off), cu(calms), n_hyp, thr, seed=seed, ns_max=int(np.diff(off).max()), polish=True))
    assert "weight_polished" not in without and not np.array_equal(_bits(without["R_t_2_polished"][1:]), _bits(out["R_t_2_polished"][1:]))


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cauchy_over_all_matches_meets_the_restatement_on_the_accuracy_scene():
    """100 matches, 30 displaced, no mask: the GPU's Cauchy adjustment at 3 px meets the restatement at 1e-9, and with it the condition that
    tests/test_ba_loss_cpu.py asserts there (less than half of least squares' rotation error)"""
    sc = bc.scene(*bc.BIG)
    ref = bc.restated(*bc.BIG, "cauchy", 3.0, False)
    off = np.array([0, bc.BIG[0]], dtype=np.int64)
    o = _ctx().bundle_adjust_ragged(sc["CalM"], sc["start"][0][None], sc["start"][1][None], np.ascontiguousarray(sc["C"]), off, loss="cauchy", scale=3.0)
    plain = _fixed(sc["C"], sc["CalM"], sc["start"], None, None, None)
    for j, (truth, key) in enumerate(zip(sc["truth"], ("R_t_2", "R_t_3"))):
        print("view %d: Cauchy %.3f deg, least squares %.3f deg" % (j + 2, bc.rot_err_deg(truth, o[key][0]), bc.rot_err_deg(truth, plain[key][0])))
    bc.gate(ref, int(o["status"][0]), int(o["iter"][0]), float(o["repr_err"][0]), o["R_t_2"][0], o["R_t_3"][0], o["Reconst"].T, o["weight"], bc.BIG)
    for truth, key in zip(sc["truth"], ("R_t_2", "R_t_3")):
        assert bc.rot_err_deg(truth, o[key][0]) < 0.5 * bc.rot_err_deg(truth, plain[key][0])
