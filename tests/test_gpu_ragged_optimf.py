"""
Ragged batches of OptimFPoseEstimation (tff_pose_batch_ragged_* with TFF_METHOD_OPTIM_F) and the refine step of robust_pose_scenes.

The contract is the ragged calls' (tests/test_gpu_ragged.py): every item's outputs -- R_t_2, R_t_3, T, its Reconst range, iter (= it1 + it2 of the
two Gauss-Helmert refinements) and status -- equal bit for bit those of the fixed-N entry point on that item, under the same context options, whatever
the batch, the neighbours, their order and n_max are.  The items sit around every routing threshold of the chain: n < 8, the exact tiers below 12, one
to many trips of 16 and of 64, and the two storage boundaries of the refinement (observations staged in LDS up to S, estimates in LDS up to L, global
slices beyond; (S, L) from tff_optim_f_ragged_bounds), plus the EPFL Fountain-P11 triplets of tests/golden/epfl_all.npz.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_ragged import _np, _bits, _fixed_by_n, _ragged_dev, _assert_item_equal   # noqa: E402

METHOD = "OptimFPoseEstimation"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _ctx(**opts):
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    ctx = api.Context(0)
    if "exact_below" in opts:
        ctx.set_exact_below(opts["exact_below"])
    if "solver" in opts:
        ctx.set_solver(opts["solver"])
    if "spill_only_if_needed" in opts:
        ctx.set_spill_only_if_needed(opts["spill_only_if_needed"])
    return ctx


def _sizes():
    from tft_vs_fund_amd import api
    S, L = api.optim_f_ragged_bounds()
    assert 0 < S < L
    return (0, 7, 8, 9, 11, 12, 13, 16, 17, 63, 64, 65, 100, 200, S, S + 1, L, L + 1, (3 * L) // 2)


@functools.lru_cache(maxsize=None)
def _data():
    """(items, (B, 9, 3) per-item CalM): three synthetic scenes of every size, every third fountain triplet; permuted so that no slot equals its item index"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    items, calms = [], []
    for k, n in enumerate(_sizes()):
        C, CalM, _, _ = generate_scene_batch(3, max(n, 1), noise=1.0, seed=300 + k)
        for b in range(3):
            items.append(np.ascontiguousarray(C[b, :n]))
            calms.append(CalM)
    d = np.load(os.path.join(GOLDEN, "epfl_all.npz"))
    off, cor, K, trip = d["fountain_offsets"], d["fountain_corresp"], d["fountain_K"], d["fountain_triplets"]
    for t in range(0, len(off) - 1, 3):
        items.append(np.ascontiguousarray(cor[off[t]:off[t + 1]]))
        calms.append(np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0))   # (1-based image numbers)
    B = len(items)
    seed = 7
    perm = np.random.default_rng(seed).permutation(B)
    while (perm == np.arange(B)).any():
        seed += 1
        perm = np.random.default_rng(seed).permutation(B)
    return [items[i] for i in perm], np.stack(calms)[perm]


def _compare(ctx, items, calms, shared, what, permute_seed=None):
    ref = _fixed_by_n(ctx, METHOD, items, calms, shared)
    o, offsets = _ragged_dev(ctx, METHOD, items, calms, shared)
    for b in range(len(items)):
        _assert_item_equal(o, offsets, b, ref[b], what)
    if permute_seed is not None:                                                 # any order of the same items: neighbours of other sizes change nothing
        perm = np.random.default_rng(permute_seed).permutation(len(items))
        o2, off2 = _ragged_dev(ctx, METHOD, [items[i] for i in perm], calms[perm] if not shared else calms, shared)
        for j, i in enumerate(perm):
            _assert_item_equal(o2, off2, j, ref[i], what + ", permuted")
    return o, ref


@pytest.mark.parametrize("shared", (True, False), ids=("shared_calm", "calm_per_item"))
def test_bitwise_equals_fixed_n(shared):
    items, calms = _data()
    ctx = _ctx()
    if shared:                                                                   # (a shared CalM is the first item's: the permuted call must keep it)
        calms = np.broadcast_to(calms[0], calms.shape).copy()
    o, ref = _compare(ctx, items, calms, shared, "ragged vs fixed-N", permute_seed=11)
    ns = np.array([len(x) for x in items])
    st, it = o["status"], o["iter"]
    print("status counts", np.bincount(st), "iter range", int(it.min()), int(it.max()))
    assert (st[ns < 8] == 1).all()
    assert (st == 0).sum() > len(items) // 2
    assert (it[(st == 0) & (ns >= 12)] > 0).all()                                # (a skipped refine stage would leave 0)


@pytest.mark.parametrize("opts", ({"exact_below": 0}, {"exact_below": 500}, {"solver": "exact"}, {"spill_only_if_needed": True}),
                         ids=("exact_below_0", "exact_below_500", "solver_exact", "spill_only_if_needed"))
def test_options_follow_fixed_n(opts):
    """the options that move the exact range (all items, none, everything below 500) and the spill boundary across the items"""
    items, calms = _data()
    _compare(_ctx(**opts), items, calms, False, "options %s" % (opts,))


def test_independent_of_the_launch():
    """every item alone (B = 1) and the batch under a doubled n_max: the classes' LDS sizes, the slices' stride and the item's neighbours change, its bits
    do not"""
    items, calms = _data()
    ctx = _ctx()
    n_top = max(len(x) for x in items)
    full, offsets = _ragged_dev(ctx, METHOD, items, calms, False, n_max=n_top)
    twice, _ = _ragged_dev(ctx, METHOD, items, calms, False, n_max=2 * n_top)
    for k in ("R_t_2", "R_t_3", "T", "Reconst"):
        assert np.array_equal(_bits(twice[k]), _bits(full[k])), "n_max doubled: %s" % k
    assert np.array_equal(twice["iter"], full["iter"]) and np.array_equal(twice["status"], full["status"])
    cm = torch.from_numpy(calms).cuda()
    for b, x in enumerate(items):
        if len(x) == 0:                                                          # (an empty packed array has no address: one row that no item owns, offsets [0, 0])
            one = _np(ctx.pose_batch_ragged(METHOD, torch.zeros((1, 6), dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"),
                                            cm[b:b + 1], n_max=0))
            torch.cuda.synchronize()
            off1 = np.zeros(2, dtype=np.int64)
        else:
            one, off1 = _ragged_dev(ctx, METHOD, [x], calms[b:b + 1], False)
        ref = dict(R_t_2=full["R_t_2"][b], R_t_3=full["R_t_3"][b], T=full["T"][b], Reconst=full["Reconst"][offsets[b]:offsets[b + 1]],
                   iter=full["iter"][b], status=full["status"][b])
        _assert_item_equal(one, off1, 0, ref, "item alone")


def test_bad_offsets():
    """a decreasing pair, a negative offset and an item above n_max get TFF_ST_BAD_OFFSETS and NaN poses; their neighbours equal the fixed-N call on the
    ranges they read"""
    from tft_vs_fund_amd import api
    items, calms = _data()
    S, L = api.optim_f_ragged_bounds()
    pick = lambda lo, hi, k: [x for x in items if lo <= len(x) <= hi][:k]
    good = pick(20, 100, 2) + pick(100, S, 2) + pick(S + 1, L, 2) + pick(L + 1, 10 ** 6, 1)     # the last one is the largest
    assert len(good) == 7 and len(good[6]) > max(len(g) for g in good[:6])
    corresp, offsets = api.pack_ragged(good)
    # item 0 starts at a negative offset and item 1 ends before it starts (offsets[2] < offsets[1]); both are refused, so no two VALID items share a
    # correspondence or a Reconst row: items 2 .. 5 keep their own ranges (a decreasing pair between two valid items would make them overlap, and the
    # shared Reconst rows would belong to whichever wrote last)
    bad_off = offsets.copy()
    bad_off[0] = -1
    bad_off[1] = offsets[2] + 1
    assert bad_off[2] < bad_off[1]
    n_max = max(len(g) for g in good[2:6])                                       # item 6 is above it
    assert len(good[6]) > n_max
    ctx = _ctx()
    ref = _fixed_by_n(ctx, METHOD, good, calms[:7], False)
    o = _np(ctx.pose_batch_ragged(METHOD, torch.from_numpy(corresp).cuda(), torch.from_numpy(bad_off).cuda(), torch.from_numpy(calms[:7]).cuda(),
                                  reconst=True, n_max=n_max))
    torch.cuda.synchronize()
    for b in (0, 1, 6):
        assert o["status"][b] == api.ST_BAD_OFFSETS and o["iter"][b] == 0
        for k in ("R_t_2", "R_t_3", "T"):
            assert np.isnan(o[k][b]).all(), (b, k)
    for b in (2, 3, 4, 5):                                                       # (observations staged in LDS: 2, 3; estimates alone in LDS: 4, 5)
        _assert_item_equal(o, offsets, b, ref[b], "neighbour of a malformed item")
    assert (o["status"][2:6] == 0).sum() >= 2
    # a malformed item leaves Reconst untouched: the rows of items 0 and 1 keep the NaN they were allocated with
    assert np.isnan(o["Reconst"][offsets[0]:offsets[2]]).all()
    # a malformed item leaves Reconst untouched: the range item 6 would own keeps the NaN it was allocated with
    assert np.isnan(o["Reconst"][offsets[6]:offsets[7]]).all()


def test_reconst_none_and_host():
    from tft_vs_fund_amd import api
    items, calms = _data()
    items, calms = items[:40], calms[:40]
    ctx = _ctx()
    o, offsets = _ragged_dev(ctx, METHOD, items, calms, False)
    o_nr, _ = _ragged_dev(ctx, METHOD, items, calms, False, reconst=False)
    assert o_nr["Reconst"] is None
    for k in ("R_t_2", "R_t_3", "T"):
        assert np.array_equal(_bits(o_nr[k]), _bits(o[k])), k
    assert np.array_equal(o_nr["status"], o["status"]) and np.array_equal(o_nr["iter"], o["iter"])
    corresp, _ = api.pack_ragged(items)
    h = ctx.pose_batch_ragged(METHOD, corresp, offsets, calms)
    for k in ("R_t_2", "R_t_3", "T", "Reconst"):
        assert np.array_equal(_bits(h[k]), _bits(o[k])), "host vs dev: %s" % k
    assert np.array_equal(h["iter"], o["iter"]) and np.array_equal(h["status"], o["status"])
    assert (h["iter"] > 0).any()


def test_oracle_parity_of_the_golden_items():
    """the items of tests/golden/optimf.npz as ONE ragged batch meet the gate of tests/test_gpu_parity.py::test_optim_f_golden (its tolerances, the same
    iteration counts, its allowance of stagnation-exit flips)"""
    from helpers import golden_cases
    from test_gpu_parity import _optimf_check
    g = np.load(os.path.join(GOLDEN, "optimf.npz"))
    e = np.load(os.path.join(GOLDEN, "epfl.npz"))
    items, calms, gold = [], [], []
    for ci, pre in golden_cases(g):
        C, CalM = g[pre + "Corresp"], g[pre + "CalM"]
        for b in range(C.shape[0]):
            items.append(np.ascontiguousarray(C[b])); calms.append(CalM)
            gold.append((g[pre + "optimf_T"][b], g[pre + "optimf_Rt2"][b], g[pre + "optimf_Rt3"][b], g[pre + "optimf_Rec"][b], g[pre + "optimf_iter"][b], (ci, b)))
    for n in range(int(e["count"])):
        pre = "t%d_" % n
        items.append(np.ascontiguousarray(e[pre + "sample"].T)); calms.append(e[pre + "CalM"])
        gold.append((g[pre + "optimf_T"], g[pre + "optimf_Rt2"], g[pre + "optimf_Rt3"], g[pre + "optimf_Rec"], g[pre + "optimf_iter"], ("epfl", n)))
    perm = np.random.default_rng(3).permutation(len(items))
    items = [items[i] for i in perm]; calms = np.stack(calms)[perm]; gold = [gold[i] for i in perm]
    o, offsets = _ragged_dev(_ctx(), METHOD, items, calms, False)
    assert (o["status"] == 0).all()
    flips = 0
    for b, (gT, gR2, gR3, gRec, git, where) in enumerate(gold):
        out = dict(T=o["T"][b:b + 1], R_t_2=o["R_t_2"][b:b + 1], R_t_3=o["R_t_3"][b:b + 1], iter=o["iter"][b:b + 1],
                   Reconst=o["Reconst"][offsets[b]:offsets[b + 1]].T[None])
        flips += _optimf_check(out, 0, gT, gR2, gR3, gRec, git, where) != 0
    assert flips <= 2


def test_scenes_refine():
    """robust_pose_scenes(..., refine="OptimFPoseEstimation"): scene s gets the bits of robust_pose(scene s, seed + s, refine=...), which runs the fixed-N
    B = 1 call on the scene's inliers; a scene with fewer matches than a sample gets ST_TOO_FEW twice; the _host path agrees with the device path"""
    from tft_vs_fund_amd import api
    from test_gpu_robust_scenes import _synthetic, _fountain, _epfl
    method = "LinearFPoseEstimation"
    sizes = np.diff(_epfl()["fountain_offsets"])
    pairs = [_synthetic(61, 9), _synthetic(5, 7), _synthetic(400, 12), _fountain(int(np.nonzero(sizes > 300)[0][0])), _synthetic(150, 11)]
    items = [a for a, _ in pairs]
    calms = np.stack([c for _, c in pairs])
    ctx = _ctx()
    kw = dict(candidates=4, lo_rounds=2)
    packed, off = api.pack_ragged(items)
    out = ctx.robust_pose_scenes(method, torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(calms).cuda(), 300, 4.0,
                                 seed=1234, ns_max=max(len(a) for a in items), refine=METHOD, polish=True, **kw)
    torch.cuda.synchronize()
    out = _np(out)
    assert out["R_t_2_refined"].shape == (5, 3, 4) and out["T_refined"].shape == (5, 3, 3, 3) and out["status_refined"].shape == (5,)
    assert "R_t_2_polished" in out
    names = ("R_t_2", "R_t_3", "T", "R_t_2_refined", "R_t_3_refined", "T_refined")
    refined_ok = 0
    for s, scene in enumerate(items):
        if scene.shape[0] < api.ROBUST_METHODS[method]:
            assert out["status"][s] == api.ST_TOO_FEW and out["status_refined"][s] == api.ST_TOO_FEW
            for k in names:
                assert np.isnan(out[k][s]).all(), (s, k)
            continue
        ref = ctx.robust_pose(method, torch.from_numpy(scene).cuda(), torch.from_numpy(calms[s]).cuda(), 300, 4.0, seed=1234 + s, refine=METHOD, **kw)
        torch.cuda.synchronize()
        for k in names:
            assert np.array_equal(_bits(out[k][s]), _bits(ref[k].cpu().numpy())), (s, k)
        assert int(out["iter_refined"][s]) == int(ref["iter_refined"]) and int(out["status_refined"][s]) == int(ref["status_refined"]), s
        assert int(out["status"][s]) == int(ref["status"]) and int(out["inliers"][s]) == int(ref["inliers"]), s
        refined_ok += int(out["status_refined"][s]) == 0 and int(out["iter_refined"][s]) > 0
    assert refined_ok >= 2
    h = ctx.robust_pose_scenes(method, packed, off, calms, 300, 4.0, seed=1234, refine=METHOD, **kw)
    for k in names:
        assert np.array_equal(_bits(h[k]), _bits(out[k])), "host vs dev: %s" % k
    assert np.array_equal(h["iter_refined"], out["iter_refined"]) and np.array_equal(h["status_refined"], out["status_refined"])
    with pytest.raises(ValueError, match="LinearTFTPoseEstimation, LinearFPoseEstimation, OptimFPoseEstimation"):
        ctx.robust_pose_scenes(method, packed, off, calms, 300, 4.0, refine="ResslTFTPoseEstimation")
