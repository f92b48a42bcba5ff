"""
Ragged, masked BundleAdjustment (tff_bundle_adjust_ragged_*, Context.bundle_adjust_ragged) and the polish of the robust estimators.

The contract is bitwise (include/tftfund.h): item b of a call gets what the EXISTING fixed-N call -- Context.bundle_adjust with B = 1 -- gives for its
selected correspondences alone.  Every comparison of poses, points and residuals here is on bit patterns, against that call.  Scenes come from
generate_scene_batch with noise, start poses and start points from LinearTFT on a parent scene of at least 12 matches (an item is a prefix of it).
Every item has its own focal length and so its own CalM (except where a shared CalM is the case under test), and the items are ordered so that an
item's slot in its launch class differs from its index: an item read with another item's calibration, pose or count does not pass.  The calls run
under both launch plans (TFF_OPT_BA_CLASSES: three classes, and the default, which is one launch for these batch sizes).
"""
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@functools.lru_cache(maxsize=None)
def _ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    ctx = api.Context(0)
    ctx.set_ba_classes(2)                                                     # three launch classes unless a test says otherwise (the default plan takes one below 257 items)
    return ctx


def _bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _np(out):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _pool(sizes, seed0, own_calm=True):
    """items of the given sizes: (corresp (n, 6), CalM, R_t_2, R_t_3 start, start points (n, 3)); the starts are LinearTFT's on the parent scene.
    own_calm: item k is seen with the focal length 38 + 3 k, so no two items share a CalM"""
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.scenes import generate_scene_batch
    parents, calms = [], []
    for k, n in enumerate(sizes):
        C, CalM, _, _ = generate_scene_batch(1, max(n, 12), noise=1.0, seed=seed0 + k, focalL=38.0 + 3.0 * k if own_calm else 50.0)
        parents.append(np.ascontiguousarray(C[0])); calms.append(np.ascontiguousarray(CalM))
    assert all(np.array_equal(calms[0], c) != own_calm for c in calms[1:])
    packed, off = api.pack_ragged(parents)
    lin = _np(_ctx().pose_batch_ragged("LinearTFTPoseEstimation", torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(),
                                       torch.from_numpy(np.stack(calms)).cuda(), reconst=True, n_max=int(np.diff(off).max())))
    assert (lin["status"] == 0).all()
    return [(parents[k][:n], calms[k], np.ascontiguousarray(lin["R_t_2"][k]), np.ascontiguousarray(lin["R_t_3"][k]),
             np.ascontiguousarray(lin["Reconst"][off[k]:off[k] + n])) for k, n in enumerate(sizes)]


def _exact_mask(n, keep, rng):
    row = np.zeros(n, dtype=np.uint8)
    row[rng.choice(n, keep, replace=False)] = rng.choice([1, 255], keep)
    return row


def _fixed(item, sel, with_x0, r2=None, r3=None):
    """the reference: the existing fixed-N call with B = 1 on the selected correspondences"""
    C, CalM, s2, s3, X0 = item
    out = _ctx().bundle_adjust(CalM, (s2 if r2 is None else r2)[None], (s3 if r3 is None else r3)[None], np.ascontiguousarray(C[sel])[None],
                               np.ascontiguousarray(X0[sel].T)[None] if with_x0 else None)
    return _np(out)


def _ragged(items, masks, with_x0, per_item_calm=True, offsets=None, r2=None, host=False, classes=2):
    from tft_vs_fund_amd import api
    packed, off = api.pack_ragged([it[0] for it in items])
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.int64)
    assert per_item_calm or all(np.array_equal(items[0][1], it[1]) for it in items)
    calm = np.stack([it[1] for it in items]) if per_item_calm else items[0][1]
    s2 = np.stack([it[2] for it in items]) if r2 is None else r2
    s3 = np.stack([it[3] for it in items])
    x0 = np.concatenate([it[4] for it in items]) if with_x0 else None
    mask = None if masks is None else np.concatenate(masks)
    if host:
        return _ctx().bundle_adjust_ragged(calm, s2, s3, packed, off, mask=mask, reconst0=x0), off
    cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert packed.shape[0] == off[-1] or offsets is not None                 # the arrays hold exactly n_total correspondences
    _ctx().set_ba_classes(classes)
    try:
        return _np(_ctx().bundle_adjust_ragged(cu(calm), cu(s2), cu(s3), cu(packed), cu(off), mask=cu(mask), reconst0=cu(x0))), off
    finally:
        _ctx().set_ba_classes(2)


def _assert_item(out, off, b, sel, ref, what):
    o0 = int(off[b])
    assert int(out["status"][b]) == int(ref["status"][0]) and int(out["iter"][b]) == int(ref["iter"][0]), (what, b)
    assert int(out["used"][b]) == int(sel.sum()), (what, b)
    for k in ("R_t_2", "R_t_3", "repr_err"):
        assert np.array_equal(_bits(out[k][b]), _bits(ref[k][0])), (what, b, k)
    rec = out["Reconst"][o0:o0 + sel.shape[0]]
    assert np.array_equal(_bits(rec[sel]), _bits(ref["Reconst"][0].T)), (what, b, "Reconst")
    assert np.isnan(rec[~sel]).all(), (what, b, "unselected")


# ---- 1. bit identity per item ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_x0", (False, True))
@pytest.mark.parametrize("mask_kind", ("none", "random", "ones"))
def test_every_item_equals_the_fixed_call(mask_kind, with_x0):
    from tft_vs_fund_amd import api
    b0 = api.ba_ragged_class_bounds()[0]
    counts = (b0 + 1, 1, 7, 12, 63, 64, 65, 200, b0)                         # item 0 is of the second class: in the first, slot = item - 1 at best
    sizes = tuple(int(np.ceil(m / 0.7)) if mask_kind == "random" else m for m in counts)
    for own_calm in (True, False):                                            # a CalM per item (calm_stride 27), one shared by the batch (calm_stride 0)
        rng = np.random.default_rng(3)
        items = _pool(sizes, 500 if mask_kind == "random" else 600, own_calm)
        masks = None if mask_kind == "none" else [_exact_mask(n, m, rng) if mask_kind == "random" else np.ones(n, dtype=np.uint8) for n, m in zip(sizes, counts)]
        sels = [np.ones(n, dtype=bool) if masks is None else masks[k] != 0 for k, n in enumerate(sizes)]
        refs = [_fixed(it, sel, with_x0) for it, sel in zip(items, sels)]
        assert all(int(r["status"][0]) == 0 for k, r in enumerate(refs) if counts[k] > 1)
        if own_calm:                                                          # the calibration matters: item 2 with item 3's CalM has other bits
            other = _fixed((items[2][0], items[3][1]) + items[2][2:], sels[2], with_x0)
            assert not np.array_equal(_bits(other["R_t_2"]), _bits(refs[2]["R_t_2"]))
        for classes in (2, 0):
            out, off = _ragged(items, masks, with_x0, own_calm, classes=classes)
            for b in range(len(items)):
                _assert_item(out, off, b, sels[b], refs[b], (mask_kind, with_x0, own_calm, classes))


# ---- 2. the upper classes --------------------------------------------------------------------------------------------------------------------------
def test_upper_classes_too_large_and_a_thinned_large_item():
    from tft_vs_fund_amd import api
    b = api.ba_ragged_class_bounds()
    assert b[2] == api.BA_MAX_N
    sizes = (12, b[1], b[1] + 1, api.BA_MAX_N, 200, api.BA_MAX_N + 200, 2 * api.BA_MAX_N)   # classes 0 1 2 2 0 - 0: slot != item in the second and third
    keep = (12, b[1], b[1] + 1, api.BA_MAX_N, 200, api.BA_MAX_N + 1, 100)
    rng = np.random.default_rng(5)
    items = _pool(sizes, 700)
    masks = [_exact_mask(n, m, rng) for n, m in zip(sizes, keep)]
    refs = {k: _fixed(items[k], masks[k] != 0, True) for k in range(len(items)) if keep[k] <= api.BA_MAX_N}
    assert all(int(r["status"][0]) == 0 for r in refs.values())
    for classes in (2, 0):
        out, off = _ragged(items, masks, True, classes=classes)
        for k in range(len(items)):
            if k not in refs:
                assert int(out["status"][k]) == api.ST_TOO_LARGE and int(out["used"][k]) == 0 and int(out["iter"][k]) == 0
                assert np.isnan(out["R_t_2"][k]).all() and np.isnan(out["R_t_3"][k]).all() and np.isnan(out["repr_err"][k])
                assert np.isnan(out["Reconst"][off[k]:off[k + 1]]).all()
                continue
            _assert_item(out, off, k, masks[k] != 0, refs[k], ("upper classes", classes))
    nomask, off = _ragged(items[:5], None, False)                            # without a mask the large items are read in place
    for k in (1, 2, 3):
        _assert_item(nomask, off, k, np.ones(sizes[k], dtype=bool), _fixed(items[k], np.ones(sizes[k], dtype=bool), False), "upper classes, no mask")


# ---- 3. failures on the device ---------------------------------------------------------------------------------------------------------------------
def test_failures_on_the_device_leave_the_neighbours_alone():
    from tft_vs_fund_amd import api
    sizes = (61, 40, 100, 30, 50, 45, 20, 10, 25)
    items = _pool(sizes, 800)
    rng = np.random.default_rng(9)
    masks = [_exact_mask(n, max(1, (7 * n) // 10), rng) for n in sizes]
    masks[7][:] = 0                                                           # nothing selected
    r2 = np.stack([it[2] for it in items]); r2[8] = np.nan                    # NaN start poses
    clean, off = _ragged(items, masks, True, r2=r2)
    ref8 = _fixed(items[8], masks[8] != 0, True, r2=r2[8])
    assert int(ref8["status"][0]) == api.ST_NONFINITE
    _assert_item(clean, off, 8, masks[8] != 0, ref8, "NaN start")
    assert int(clean["status"][7]) == api.ST_TOO_FEW and int(clean["used"][7]) == 0 and np.isnan(clean["R_t_2"][7]).all() and np.isnan(clean["repr_err"][7])
    assert (clean["status"][:7] == 0).all()
    bad = off.copy()
    bad[0] = -1                                                               # item 0: negative
    bad[3] = off[4] + 5                                                       # item 2 grows over item 3 and five matches of item 4; item 3 decreases
    bad[9] = off[9] + 1                                                       # item 8: beyond n_total
    out, _ = _ragged(items, masks, True, r2=r2, offsets=bad)
    for b in (0, 3, 8):
        assert int(out["status"][b]) == api.ST_BAD_OFFSETS and int(out["used"][b]) == 0 and int(out["iter"][b]) == 0, b
        assert np.isnan(out["R_t_2"][b]).all() and np.isnan(out["R_t_3"][b]).all() and np.isnan(out["repr_err"][b]), b
    allmask = np.concatenate(masks)
    for b in (1, 4, 5, 6):                                                    # the neighbours: the bits of the clean run (item 4 shares five positions of Reconst with item 2)
        for k in ("R_t_2", "R_t_3", "repr_err"):
            assert np.array_equal(_bits(out[k][b]), _bits(clean[k][b])), (b, k)
        assert out["iter"][b] == clean["iter"][b] and out["status"][b] == clean["status"][b] and out["used"][b] == clean["used"][b]
        lo = int(off[b]) + (5 if b == 4 else 0)                               # (item 2 writes the first five positions of item 4 too)
        assert np.array_equal(_bits(out["Reconst"][lo:off[b + 1]]), _bits(clean["Reconst"][lo:off[b + 1]])), b
    assert int(out["status"][7]) == api.ST_TOO_FEW
    sel2 = allmask[bad[2]:bad[3]] != 0                                        # item 2 as the offsets now state it
    big = (np.concatenate([it[0] for it in items])[bad[2]:bad[3]], items[2][1], items[2][2], items[2][3], np.concatenate([it[4] for it in items])[bad[2]:bad[3]])
    ref2 = _fixed(big, sel2, True)
    assert int(out["used"][2]) == int(sel2.sum()) and np.array_equal(_bits(out["R_t_2"][2]), _bits(ref2["R_t_2"][0])) and out["iter"][2] == ref2["iter"][0]


# ---- 4. the _host form ------------------------------------------------------------------------------------------------------------------------------
def test_host_form():
    from tft_vs_fund_amd import api
    ctx = _ctx()
    sizes = (61, 7, 200, 30)
    items = _pool(sizes, 900)
    rng = np.random.default_rng(11)
    masks = [_exact_mask(n, max(1, (7 * n) // 10), rng) for n in sizes]
    for mk, with_x0 in ((masks, True), (None, False)):
        dev, off = _ragged(items, mk, with_x0)
        host, _ = _ragged(items, mk, with_x0, host=True)
        assert isinstance(host["Reconst"], np.ndarray) and host["R_t_2"].shape == (4, 3, 4)
        for k in ("R_t_2", "R_t_3", "repr_err", "Reconst"):
            assert np.array_equal(_bits(host[k]), _bits(dev[k])), k
        for k in ("iter", "status", "used"):
            assert np.array_equal(host[k], dev[k]), k
    # the C entry point itself: malformed offsets are refused before any work; every optional pointer may be NULL
    packed, off = api.pack_ragged([it[0] for it in items])
    calm = np.ascontiguousarray(np.stack([it[1].T.reshape(27) for it in items]))      # a CalM per item, column-major
    cm = lambda R: np.ascontiguousarray(np.stack(R).transpose(0, 2, 1)).reshape(-1)
    r2 = cm([it[2] for it in items]); r3 = cm([it[3] for it in items])
    o2 = np.zeros(4 * 12); o3 = np.zeros(4 * 12)
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    call = lambda o: ctx.lib.tff_bundle_adjust_ragged_host(ctx.handle, p(packed), p(o), None, p(calm), 27, p(r2), p(r3), None, 4, p(o2), p(o3), None, None, None,
                                                           None, None)
    assert call(off) == 0
    assert np.array_equal(_bits(o2.reshape(4, 4, 3).transpose(0, 2, 1)), _bits(dev["R_t_2"]))
    for broken in (np.array([0, 70, 61, 268, 298]), np.array([-1, 61, 68, 268, 298])):
        assert call(np.ascontiguousarray(broken, dtype=np.int64)) == -10001    # TFF_E_INVALID
    with pytest.raises(ValueError):
        ctx.bundle_adjust_ragged(np.stack([it[1] for it in items]), np.stack([it[2] for it in items]), np.stack([it[3] for it in items]), packed, np.array([0, 70, 61, 268, 298]))


# ---- 5. robust -> polish, end to end ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fountain_with_outliers():
    """six fountain triplets of ~100 .. 1 400 matches, a quarter of each displaced by U(20, 80) px in views 2, 3 (the recipe of tests/test_gpu_robust_scenes.py).
    The dataset's cameras share one K, so scene k is resampled to another pixel size (coordinates and K scaled by s_k): a CalM per scene that differs"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epfl_all.npz"))
    off, K, trip = d["fountain_offsets"], d["fountain_K"], d["fountain_triplets"]
    n = np.diff(off)
    picks = [int(np.argmin(np.abs(n - want))) for want in (100, 150, 250, 400, 700, 1400)]
    assert len(set(picks)) == 6
    scenes, calms = [], []
    for k, t in enumerate(picks):
        sc = np.array(d["fountain_corresp"][off[t]:off[t + 1]], dtype=np.float64)
        rng = np.random.default_rng(300 + k)
        bad = rng.choice(sc.shape[0], sc.shape[0] // 4, replace=False)
        sc[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
        px = (1.0, 0.9, 1.1, 0.95, 1.05, 1.15)[k]
        scenes.append(np.ascontiguousarray(px * sc)); calms.append(np.concatenate([np.diag([px, px, 1.0]) @ K[v - 1] for v in trip[t][:3]], axis=0))
    assert all(not np.array_equal(calms[0], c) for c in calms[1:])
    return scenes, np.stack(calms)


def test_robust_scenes_polish_end_to_end():
    from oracle import ba_oracle as BA
    from tft_vs_fund_amd import api
    ctx = _ctx()
    scenes, calms = _fountain_with_outliers()
    packed, off = api.pack_ragged(scenes)
    args = ("LinearTFTPoseEstimation", torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(calms).cuda(), 1001, 4.0)
    kw = dict(seed=21, candidates=4, lo_rounds=2, ns_max=int(np.diff(off).max()))
    plain = _np(ctx.robust_pose_scenes(*args, **kw))
    out = _np(ctx.robust_pose_scenes(*args, polish=True, **kw))
    assert (out["status"] == 0).all()
    for k in plain:                                                           # the robust result itself is untouched
        same = np.array_equal(_bits(out[k]), _bits(plain[k])) if plain[k].dtype == np.float64 else np.array_equal(out[k], plain[k])
        assert same, k
    ba = _np(ctx.bundle_adjust_ragged(args[3], torch.from_numpy(out["R_t_2"]).cuda(), torch.from_numpy(out["R_t_3"]).cuda(), args[1], args[2],
                                      mask=torch.from_numpy(out["mask"]).cuda(), reconst=False))
    assert np.array_equal(ba["used"], out["inliers"]) and ba["Reconst"] is None
    # (a polish may end as the fixed-N call ends on those matches, TFF_ST_NONFINITE included: the comparison below is bitwise either way; the oracle is
    # asked about the two smallest scenes whose BundleAdjustment finishes)
    finished = [int(s) for s in np.argsort([sc.shape[0] for sc in scenes]) if out["status_polished"][s] == 0]
    print("inliers", out["inliers"].tolist(), "status_polished", out["status_polished"].tolist(), "iter_polished", out["iter_polished"].tolist())
    assert len(finished) >= 2
    for s in range(6):
        sel = out["mask"][off[s]:off[s + 1]] != 0
        ref = _np(ctx.bundle_adjust(calms[s], out["R_t_2"][s][None], out["R_t_3"][s][None], np.ascontiguousarray(scenes[s][sel])[None], None))
        for k in ("R_t_2", "R_t_3", "repr_err"):
            assert np.array_equal(_bits(out[k + "_polished"][s]), _bits(ref[k][0])) and np.array_equal(_bits(ba[k][s]), _bits(ref[k][0])), (s, k)
        assert out["iter_polished"][s] == ref["iter"][0] and out["status_polished"][s] == ref["status"][0]
        if s in finished[:2]:                                                 # against the numpy statement of BundleAdjustment.m
            R_t_0 = np.vstack([np.eye(3, 4), out["R_t_2"][s], out["R_t_3"][s]])
            Ro, _, ito, erro = BA.BundleAdjustment(calms[s], R_t_0, scenes[s][sel].T.copy(), None)
            rel = lambda a, r: np.abs(a - r).max() / np.abs(r).max()
            e2, e3, ee = rel(out["R_t_2_polished"][s], Ro[3:6]), rel(out["R_t_3_polished"][s], Ro[6:9]), abs(out["repr_err_polished"][s] - erro) / erro
            print("scene %d: %d inliers, iter %d / oracle %d, deviations %.2e %.2e %.2e" % (s, int(sel.sum()), out["iter_polished"][s], ito, e2, e3, ee))
            assert out["iter_polished"][s] == ito and e2 < 1e-9 and e3 < 1e-9 and ee <= 1e-9
    # one scene: the offsets are [0, Ns]
    one = _np(ctx.robust_pose("LinearTFTPoseEstimation", torch.from_numpy(scenes[0]).cuda(), torch.from_numpy(calms[0]).cuda(), 1001, 4.0, seed=21, candidates=4,
                              lo_rounds=2, polish=True))
    for k in ("R_t_2", "R_t_3", "repr_err"):
        assert np.array_equal(_bits(one[k + "_polished"]), _bits(out[k + "_polished"][0])), k
    assert int(one["iter_polished"]) == int(out["iter_polished"][0]) and int(one["status_polished"]) == int(out["status_polished"][0])
