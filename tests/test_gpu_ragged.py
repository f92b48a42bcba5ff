"""
Ragged batches (tff_pose_batch_ragged_*): one call for triplets with different correspondence counts.  The contract is bitwise: every
triplet's outputs -- R_t_2, R_t_3, T, its Reconst range, iter, status -- equal those of the fixed-N entry point on that triplet, under the
same context options.  The items mix synthetic scenes around every routing threshold (n < 7 / 8, exact tiers below 12, LDS staging
limits of the fix-up kernels, one to many trips of 16) with the EPFL Fountain-P11 triplets of tests/golden/epfl_all.npz (1 .. 1 400
correspondences each).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

METHODS = ("LinearTFTPoseEstimation", "LinearFPoseEstimation")
SIZES = (0, 5, 6, 7, 8, 9, 11, 12, 13, 31, 64, 100, 199, 200, 201, 257, 400, 1000)


def _ctx(**opts):
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    ctx = api.Context(0)
    if "exact_below" in opts:
        ctx.set_exact_below(opts["exact_below"])
    if "solver" in opts:
        ctx.set_solver(opts["solver"])
    return ctx


def _items():
    """(list of (n, 6) arrays, (B, 9, 3) per-item CalM) -- synthetic scenes of every size in SIZES, then the fountain triplets."""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    import os
    items, calms = [], []
    for k, n in enumerate(SIZES):
        C, CalM, _, _ = generate_scene_batch(3, max(n, 1), noise=1.0, seed=100 + k)
        for b in range(3):
            items.append(np.ascontiguousarray(C[b, :n]))
            calms.append(CalM)
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epfl_all.npz"))
    off, cor, K, trip = d["fountain_offsets"], d["fountain_corresp"], d["fountain_K"], d["fountain_triplets"]
    for t in range(0, len(off) - 1, 3):
        items.append(np.ascontiguousarray(cor[off[t]:off[t + 1]]))
        calms.append(np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0))   # (1-based image numbers)
    return items, np.stack(calms)


def _np(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in o.items() if k != "_raw"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _fixed_empty(ctx, method, B, cm):
    """the fixed-N _dev call with N = 0 (a valid, non-null corresp pointer that is never read; Reconst has no entries)"""
    from tft_vs_fund_amd import api
    dev = torch.device("cuda", 0)
    dummy = torch.zeros(6, dtype=torch.float64, device=dev)
    cm_cm = cm.t().contiguous().reshape(27) if cm.dim() == 2 else cm.transpose(1, 2).contiguous().reshape(B * 27)
    Rt2 = torch.empty((B, 12), dtype=torch.float64, device=dev); Rt3 = torch.empty_like(Rt2)
    T = torch.empty((B, 27), dtype=torch.float64, device=dev)
    it = torch.zeros(B, dtype=torch.int32, device=dev); st = torch.zeros(B, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    fn = getattr(ctx.lib, api.POSE_METHODS[method] + "_dev")
    assert fn(ctx.handle, p(dummy), p(cm_cm), 0 if cm.dim() == 2 else 27, B, 0, p(Rt2), p(Rt3), p(T), None, p(it), p(st)) == 0
    torch.cuda.synchronize()
    return dict(R_t_2=Rt2.cpu().numpy().reshape(B, 4, 3).transpose(0, 2, 1), R_t_3=Rt3.cpu().numpy().reshape(B, 4, 3).transpose(0, 2, 1),
                T=T.cpu().numpy().reshape(B, 3, 3, 3).transpose(0, 3, 2, 1), Reconst=np.zeros((B, 3, 0)), iter=it.cpu().numpy(),
                status=st.cpu().numpy())


def _fixed_by_n(ctx, method, items, calms, shared):
    """reference: the fixed-N _dev call on the items of each n, per item"""
    ref = [None] * len(items)
    ns = np.array([len(x) for x in items])
    for n in np.unique(ns):
        idx = np.nonzero(ns == n)[0]
        cm = torch.from_numpy(calms[0] if shared else calms[idx]).cuda()
        if n == 0:
            o = _fixed_empty(ctx, method, len(idx), cm)
        else:
            C = torch.from_numpy(np.ascontiguousarray(np.stack([items[i] for i in idx]).reshape(len(idx), n, 6))).cuda()
            o = _np(ctx.pose_batch(method, C, cm, reconst=True))
        torch.cuda.synchronize()
        for j, i in enumerate(idx):
            ref[i] = dict(R_t_2=o["R_t_2"][j], R_t_3=o["R_t_3"][j], T=o["T"][j], Reconst=o["Reconst"][j].T, iter=o["iter"][j],
                          status=o["status"][j])
    return ref


def _ragged_dev(ctx, method, items, calms, shared, n_max=None, reconst=True):
    from tft_vs_fund_amd import api
    corresp, offsets = api.pack_ragged(items)
    cm = torch.from_numpy(calms[0] if shared else calms).cuda()
    o = _np(ctx.pose_batch_ragged(method, torch.from_numpy(corresp).cuda(), torch.from_numpy(offsets).cuda(), cm, reconst=reconst, n_max=n_max))
    torch.cuda.synchronize()
    return o, offsets


def _assert_item_equal(o, offsets, b, ref, what):
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(o[k][b]), _bits(ref[k])), "%s: item %d, %s differs" % (what, b, k)
    if o.get("Reconst") is not None:
        assert np.array_equal(_bits(o["Reconst"][offsets[b]:offsets[b + 1]]), _bits(ref["Reconst"])), "%s: item %d, Reconst differs" % (what, b)
    assert o["iter"][b] == ref["iter"] and o["status"][b] == ref["status"], "%s: item %d, iter/status differ" % (what, b)


@pytest.fixture(scope="module")
def data():
    items, calms = _items()
    perm = np.random.default_rng(7).permutation(len(items))
    return [items[i] for i in perm], calms[perm]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shared", (True, False))
def test_ragged_bitwise_equals_fixed_n(data, method, shared):
    items, calms = data
    ctx = _ctx()
    ref = _fixed_by_n(ctx, method, items, calms, shared)
    o, offsets = _ragged_dev(ctx, method, items, calms, shared)
    for b in range(len(items)):
        _assert_item_equal(o, offsets, b, ref[b], "ragged vs fixed-N")
    st = o["status"]
    assert (st[[i for i, x in enumerate(items) if len(x) < 7]] == 1).all()
    assert (st == 0).sum() > len(items) // 2
    # any order of the same items: wavefront neighbours of other sizes change nothing
    perm = np.random.default_rng(11).permutation(len(items))
    o2, off2 = _ragged_dev(ctx, method, [items[i] for i in perm], calms[perm], shared)
    for j, i in enumerate(perm):
        _assert_item_equal(o2, off2, j, ref[i], "permuted")


@pytest.mark.parametrize("method", METHODS)
def test_ragged_host_and_null_outputs(data, method):
    from tft_vs_fund_amd import api
    items, calms = data
    items, calms = items[:40], calms[:40]
    ctx = _ctx()
    o, offsets = _ragged_dev(ctx, method, items, calms, False)
    corresp, _ = api.pack_ragged(items)
    h = ctx.pose_batch_ragged(method, corresp, offsets, calms)
    for k in ("R_t_2", "R_t_3", "T", "Reconst"):
        assert np.array_equal(_bits(h[k]), _bits(o[k])), "host vs dev: %s" % k
    assert np.array_equal(h["iter"], o["iter"]) and np.array_equal(h["status"], o["status"])
    # reconst = NULL, then iter = status = NULL
    o_nr, _ = _ragged_dev(ctx, method, items, calms, False, reconst=False)
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(o_nr[k]), _bits(o[k]))
    assert np.array_equal(o_nr["status"], o["status"])
    B = len(items)
    dev = torch.device("cuda", 0)
    C = torch.from_numpy(corresp).cuda(); off = torch.from_numpy(offsets).cuda()
    cm = torch.from_numpy(calms).cuda().transpose(1, 2).contiguous().reshape(B * 27)
    Rt2 = torch.empty((B, 12), dtype=torch.float64, device=dev); Rt3 = torch.empty_like(Rt2)
    T = torch.empty((B, 27), dtype=torch.float64, device=dev)
    rec = torch.full((corresp.shape[0], 3), float("nan"), dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    rc = ctx.lib.tff_pose_batch_ragged_dev(ctx.handle, api.METHOD_IDS[method], p(C), p(off), int(np.diff(offsets).max()), p(cm), 27, B,
                                           p(Rt2), p(Rt3), p(T), p(rec), None, None)
    assert rc == 0, ctx.lib.tff_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(T.cpu().numpy().reshape(B, 3, 3, 3).transpose(0, 3, 2, 1)), _bits(o["T"]))
    assert np.array_equal(_bits(rec.cpu().numpy()), _bits(o["Reconst"]))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("opts", ({"exact_below": 0}, {"solver": "exact"}), ids=("exact_below_0", "solver_exact"))
def test_ragged_options_follow_fixed_n(data, method, opts):
    items, calms = data
    items = [x for x in items if len(x) <= 400][:60]
    calms = calms[:len(items)]
    ctx = _ctx(**opts)
    ref = _fixed_by_n(ctx, method, items, calms, True)
    o, offsets = _ragged_dev(ctx, method, items, calms, True)
    for b in range(len(items)):
        _assert_item_equal(o, offsets, b, ref[b], "options %s" % opts)


def test_ragged_bad_offsets_and_refusals(data):
    from tft_vs_fund_amd import api
    items, calms = data
    good = [x for x in items if 20 <= len(x) <= 300][:6]
    corresp, offsets = api.pack_ragged(good)
    ctx = _ctx()
    method = "LinearTFTPoseEstimation"
    # item 2 made malformed: it ends before it starts (offsets[3] < offsets[2]); the others keep their offsets, so item 3 now holds the
    # correspondences P[offsets[2] - 1 : offsets[4]] -- the reference for each neighbour is a clean call on the ranges it reads
    bad_off = offsets.copy()
    bad_off[3] = offsets[2] - 1
    segs = [corresp[bad_off[b]:bad_off[b + 1]] if b != 2 else corresp[offsets[2]:offsets[3]] for b in range(len(good))]
    bad_corr = corresp
    clean, _ = _ragged_dev(ctx, method, segs, calms, True, reconst=False)
    assert bad_off[3] < bad_off[2]
    cm = torch.from_numpy(calms[0]).cuda()
    o = _np(ctx.pose_batch_ragged(method, torch.from_numpy(bad_corr).cuda(), torch.from_numpy(bad_off).cuda(), cm, reconst=False,
                                  n_max=int(max(len(g) for g in segs))))
    torch.cuda.synchronize()
    assert o["status"][2] == api.ST_BAD_OFFSETS and np.isnan(o["T"][2]).all() and np.isnan(o["R_t_2"][2]).all()
    for b in (0, 1, 3, 4, 5):
        for k in ("R_t_2", "R_t_3", "T"):
            assert np.array_equal(_bits(o[k][b]), _bits(clean[k][b])), (b, k)
        assert o["status"][b] == clean["status"][b] and o["iter"][b] == clean["iter"][b]
    # n_b > n_max: only the items above the bound are refused
    clean, _ = _ragged_dev(ctx, method, good, calms, True, reconst=False)
    n_max = int(sorted(len(g) for g in good)[3])
    o, _ = _ragged_dev(ctx, method, good, calms, True, n_max=n_max, reconst=False)
    for b, g in enumerate(good):
        if len(g) > n_max:
            assert o["status"][b] == api.ST_BAD_OFFSETS and np.isnan(o["R_t_3"][b]).all()
        else:
            assert np.array_equal(_bits(o["T"][b]), _bits(clean["T"][b])) and o["status"][b] == clean["status"][b]
    # host path: malformed offsets are refused before any work
    with pytest.raises(ValueError):
        ctx.pose_batch_ragged(method, bad_corr, bad_off, calms[0])
    rc = ctx.lib.tff_pose_batch_ragged_host(ctx.handle, 0, ctypes.c_void_p(bad_corr.ctypes.data), ctypes.c_void_p(bad_off.ctypes.data),
                                            ctypes.c_void_p(np.ascontiguousarray(calms[0].T).ctypes.data), 0, len(good), None, None, None, None,
                                            None, None)
    assert rc == -10001
    # B = 0 returns 0; n_max < 0, NULL offsets, an unknown method, TFF_OPT_ROWS = 0, an iterative method: TFF_E_INVALID
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    zc = torch.zeros((1, 6), dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert ctx.lib.tff_pose_batch_ragged_dev(ctx.handle, 0, p(zc), p(z), 0, p(cm), 0, 0, None, None, None, None, None, None) == 0
    assert ctx.lib.tff_pose_batch_ragged_dev(ctx.handle, 0, p(zc), p(z), -1, p(cm), 0, 0, None, None, None, None, None, None) == -10001
    assert ctx.lib.tff_pose_batch_ragged_dev(ctx.handle, 0, p(zc), None, 0, p(cm), 0, 0, None, None, None, None, None, None) == -10001
    assert ctx.lib.tff_pose_batch_ragged_dev(ctx.handle, 9, p(zc), p(z), 0, p(cm), 0, 0, None, None, None, None, None, None) == -10001
    with pytest.raises(api.TffError):
        _ragged_dev(ctx, "ResslTFTPoseEstimation", good, calms, True)
    ctx.set_rows(0)
    with pytest.raises(api.TffError, match="TFF_OPT_ROWS"):
        _ragged_dev(ctx, method, good, calms, True)


def _retry_batch():
    """a ragged batch that reaches the exact fix-up: several thousand noisy minimal samples (n = 7, and n = 8 for LinearF) among
    well-posed triplets of other sizes, shuffled"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    items = []
    for n, B, noise, seed in ((7, 3000, 3.0, 5), (8, 2000, 3.0, 6), (12, 300, 3.0, 7), (40, 300, 1.0, 8), (150, 200, 1.0, 9), (260, 100, 1.0, 10)):
        C, CalM, _, _ = generate_scene_batch(B, n, noise=noise, seed=seed)
        items += [np.ascontiguousarray(C[b]) for b in range(B)]
    perm = np.random.default_rng(13).permutation(len(items))
    return [items[i] for i in perm], CalM


@pytest.mark.parametrize("stage_lds", (-1, 0, 1), ids=("stage_auto", "stage_off", "stage_on"))
@pytest.mark.parametrize("method", METHODS)
def test_ragged_exact_fixup_bitwise_equals_fixed_n(method, stage_lds):
    """TFF_OPT_EXACT_BELOW = 0: the row kernels flag what their fast tiers cannot finish and the one-triplet exact kernel redoes it from the
    retry list -- in ragged mode with each triplet's own n, first correspondence, Reconst rows and LDS staging decision.  Every triplet's
    outputs equal the fixed-N call's bit for bit, under each TFF_OPT_STAGE_LDS setting (the fix-up's staging bound and LDS size)."""
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    items, CalM = _retry_batch()
    ctx = api.Context(0, stage_lds=stage_lds)
    ctx.set_exact_below(0)
    calms = CalM[None]
    ref = _fixed_by_n(ctx, method, items, calms, True)
    o, offsets = _ragged_dev(ctx, method, items, calms, True)
    for b in range(len(items)):
        _assert_item_equal(o, offsets, b, ref[b], "fix-up, stage_lds=%d" % stage_lds)
    if method == "LinearTFTPoseEstimation":
        # the fixed-N route of these triplets does reach the exact kernel (it stamps its iteration count + 10000 into dbg[69])
        ctx.set_debug_adaptive(True)
        C = torch.from_numpy(np.stack([x for x in items if len(x) == 7])).cuda()
        dbg = ctx.pose_batch(method, C, torch.from_numpy(CalM).cuda(), reconst=False, debug=True)["debug"].cpu().numpy()
        assert (dbg[:, 69] >= 10000).sum() > 0
