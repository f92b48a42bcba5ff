"""
Per-view calibration, unseen camera rigs and N > 4096 on the MI355X, through every entry point that takes a CalM (cases: tests/rig_cases.py).

Every other input of the suite comes from one K for all views (CalM = [K; K; K], zero skew, K(3,3) = 1) and one rig of three converging cameras.  With
K1 = K2 = K3 the calibration index is periodic in the view, so reading K2 where K3 is meant, building E = K2' F K1 from the wrong pair, a per-scene
calm_stride off by a view or a reordered block in the API layer change no bit of any output.  Here the three blocks of CalM differ in focal length
(> 20 %), principal point, skew (either sign) and overall scale (K(3,3) != 1) and differ between the items of a batch; the rigs add parallel optical
axes (epipoles at infinity), forward motion (epipole at the principal point), cameras rolled by 100 and 180 degrees and collinear centres with parallel
axes; and N = 4096 / 4097 sit on both sides of the switch in pose_common.h::recover_vote (two vote scores packed into 16-bit halves / two single passes).

References: oracle/tft_oracle.py and oracle/ba_oracle.py (numpy, LAPACK) with the calibration of each view, at the project's existing gates -- 1e-9 for
the linear paths and BundleAdjustment, 1e-8 and the same `iter` for OptimF -- and bitwise contracts where the library states one.  Every oracle
comparison carries a control: the same reference with K2 and K3 exchanged (rig_cases.swap_views_23) must be further than 1e-3 from the result, which
proves that the case can see a view mix-up.  Measured figures: profiles/rigs_parity.txt.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import rig_cases as RC                                   # noqa: E402
from helpers import rel_err, rel_err_T, pose_err_any_convention   # noqa: E402

TOL_LINEAR = 1e-9          # TOL of tests/test_gpu_rows.py and tests/test_gpu_blocks.py
TOL_OPTIMF = 1e-8          # tests/test_emulated_kernels.py::test_optim_f_kernel_matches_golden
TOL_BA = 1e-9              # the BundleAdjustment gate of the README
LINEAR = ["LinearTFTPoseEstimation", "LinearFPoseEstimation"]


def _O():
    from oracle import tft_oracle as O
    return O


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _pose(ctx, method, C, CalM, reconst=True, debug=False):
    out = ctx.pose_batch(method, _dev(C), _dev(CalM), reconst=reconst, debug=debug)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items() if k != "_raw" and v is not None}


def _report(test, **figures):
    """the figures of profiles/rigs_parity.txt: printed (pytest -s shows them), one line per test"""
    print("rigs_parity %s %s" % (test, " ".join("%s=%.3e" % kv for kv in sorted(figures.items()))))


@pytest.fixture(scope="module")
def ctx():
    """a context with the library's defaults, for the entry points that do not take a route"""
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    return api.Context(0)


# ---- a. linear paths and OptimF, fixed N ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixed_n_case(method, rig, K, B, N, tol):
    """(Corresp, CalM, oracle references), computed once and shared by the two routes; items the oracle itself cannot hold to the gate are redrawn
    (rig_cases.well_posed_batch: a criterion on the reference alone)"""
    C, CalM, _, _, _ = RC.well_posed_batch(rig, B, N, 0.5, 2000 + N, K, method, tol)
    return C, CalM, RC.oracle_refs(method, C, CalM)


@pytest.mark.parametrize("K", ["per_view", "shared"])
@pytest.mark.parametrize("rig", RC.RIGS)
@pytest.mark.parametrize("method", LINEAR + ["OptimFPoseEstimation"])
def test_fixed_n_poses_against_the_oracle(gpu_ctx, method, rig, K):
    """B = 9 (two full four-triplet wavefronts and a tail of one), N = the exact tier (7 / 8), 12, 49 (just above STAGE_MAX_N_F) and 201 (just above
    STAGE_MAX_N_TFT), noise 0.5 px, Reconst requested; CalM (B, 9, 3) with every block different, or (9, 3) with three different blocks.  OptimF has no
    debug record in the library: the tie rule reads the oracle's vote scores for it (rig_cases.check_pose_batch)."""
    B = 9
    optim = method == "OptimFPoseEstimation"
    worst, control = 0.0, np.inf
    for N in (7 if method == "LinearTFTPoseEstimation" else 8, 12, 49, 201):
        tol = TOL_OPTIMF if optim else TOL_LINEAR
        C, CalM, refs = _fixed_n_case(method, rig, K, B, N, tol)
        out = _pose(gpu_ctx, method, C, CalM)
        votes = None if optim else _pose(gpu_ctx, method, C, CalM, debug=True)["debug"][:, 60:68]
        w, c = RC.check_pose_batch(out, method, C, CalM, tol, refs, votes=votes, same_iter=optim,
                                   what="%s %s %s N=%d route %d" % (method, rig, K, N, gpu_ctx.route))
        worst, control = max(worst, w), min(control, c)
    _report("a.%s.%s.%s.route%d" % (method, rig, K, gpu_ctx.route), worst=worst, control=control)


# ---- b. the five Gauss-Helmert trifocal methods ----------------------------------------------------------------------------------------------------------
GH_METHODS = ["ResslTFTPoseEstimation", "NordbergTFTPoseEstimation", "FaugPapaTFTPoseEstimation", "PiPoseEstimation", "PiColPoseEstimation"]


@pytest.mark.parametrize("rig", ["converging", "parallel"])
@pytest.mark.parametrize("method", GH_METHODS)
def test_iterative_trifocal_methods_use_calm_after_the_iteration_only(gpu_ctx, method, rig):
    """The LAPACK oracle cannot gate their iteration (1e-7 .. 1e-4, README; the 50-digit gates of tests/test_gpu_gh_noise.py do), so this asserts what
    CalM can and cannot touch: the poses are R_t_from_TFT of the kernel's own T with the calibration of each view, Reconst the triangulation with
    those poses, the control with K2 and K3 exchanged is far away, and T, iter and status do not change by a bit when CalM = [K1; K1; K1]
    (CalM enters after the iteration, as in ResslTFTPoseEstimation.m).  PiCol runs on the collinear twin of each rig.

    This test found a loss of six digits, since fixed: PiCol on converging_collinear, N = 12, item 7 of 9 sat at 1.44e-9 (t3; rotations 1.6e-10 and
    3.9e-10) on both routes while every other method and rig stayed below 5e-13.  With collinear centres a slice of the calibrated tensor is nearly of
    rank one (singular values 0.70, 5e-6, 0 for this item); a 50-digit evaluation of R_t_from_TFT at the kernel's T agreed with the LAPACK oracle to
    4e-15 and with the kernel to 2.6e-10 / 7.1e-10.  csrc/small_la.h::null3 took the slice's null vector from the formed M'M on its exact tier too; it
    now hands a slice whose gap is below 1e-7 tr to the one-sided Jacobi on M itself (the item: 2.3e-12)."""
    O = _O()
    B = 9
    if method == "PiColPoseEstimation":
        rig = {"converging": "converging_collinear", "parallel": "collinear_parallel"}[rig]
    worst, control = 0.0, np.inf
    for N in (12, 40):
        C, CalM, _, _, _ = RC.well_posed_batch(rig, B, N, 0.5, 3000 + N, "per_view", "LinearTFTPoseEstimation", 1e-9)   # (R_t_from_TFT well-posed at the linear T)
        out = _pose(gpu_ctx, method, C, CalM)
        same_k = _pose(gpu_ctx, method, C, RC.first_view_only(CalM))
        assert np.all(out["status"] == 0), (method, rig, N, out["status"].tolist())
        for k in ("T", "iter", "status"):
            assert np.array_equal(out[k], same_k[k]), (method, rig, N, k)
        for b in range(B):
            Cb = C[b].T.copy()
            R2, R3 = O.R_t_from_TFT(out["T"][b], CalM[b], Cb)
            e = max(rel_err(out["R_t_2"][b], R2), rel_err(out["R_t_3"][b], R3), rel_err(out["Reconst"][b], O._final_reconst(CalM[b], R2, R3, Cb)))
            assert e < 1e-9, "%s %s N=%d item %d: poses / Reconst %.3e from R_t_from_TFT of the kernel's own T (gate 1e-9)" % (method, rig, N, b, e)
            S2, S3 = O.R_t_from_TFT(out["T"][b], RC.swap_views_23(CalM[b]), Cb)
            d = max(rel_err(out["R_t_2"][b], S2), rel_err(out["R_t_3"][b], S3))
            assert d > 1e-3, (method, rig, N, b, d)
            worst, control = max(worst, e), min(control, d)
    _report("b.%s.%s.route%d" % (method, rig, gpu_ctx.route), worst=worst, control=control)


# ---- c. ragged and sampled forms ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", LINEAR + ["OptimFPoseEstimation"])
def test_ragged_items_equal_their_fixed_n_calls(ctx, method):
    """pose_batch_ragged with one CalM per item and n = 8, 12, 49, 201 mixed in one call: every item bit for bit what pose_batch gives for it alone with
    its own CalM (the contract of tests/test_gpu_ragged.py, which holds only if item b reads calm + 27 b).  Ragged batches run on the row kernels only
    (TFF_OPT_ROWS = 0 is refused), so this runs on a context with the library's defaults."""
    gpu_ctx = ctx
    from tft_vs_fund_amd import api
    sizes = [8, 201, 12, 49, 12, 8, 49, 201, 12]
    rigs = ["roll", "parallel", "forward", "converging", "collinear_parallel"]
    CalM = RC.per_view_calm(len(sizes))
    items = [RC.rig_batch(rigs[b % 5], 1, n, 0.5, seed=400 + b, K=CalM[b])[0][0] for b, n in enumerate(sizes)]
    packed, off = api.pack_ragged(items)
    out = gpu_ctx.pose_batch_ragged(method, _dev(packed), _dev(off), _dev(CalM), reconst=True)
    torch.cuda.synchronize()
    out = {k: _np(v) for k, v in out.items() if k != "_raw"}
    assert np.all(out["status"] == 0)
    for b, item in enumerate(items):
        one = _pose(gpu_ctx, method, item[None], CalM[b])
        for k in ("T", "R_t_2", "R_t_3", "iter", "status"):
            assert np.array_equal(out[k][b], one[k][0]), (method, b, k)
        assert np.array_equal(out["Reconst"][off[b]:off[b + 1]].T, one["Reconst"][0]), (method, b)
        # (and the item alone is the oracle's with its own calibration: case a, same kernels)


@pytest.mark.parametrize("method,n", [("LinearTFTPoseEstimation", 7), ("LinearFPoseEstimation", 8)])
def test_sampled_hypotheses_with_per_view_calibration(gpu_ctx, method, n):
    """pose_sampled, 96 minimal samples of a parallel-rig scene of 240 exact matches, a quarter of them displaced, three different K: every sixth hypothesis
    against the oracle at 1e-6; a cheirality tie is held to the best sign convention of svd(E), at most two of them
    (tests/test_gpu_blocks.py::test_config4_minimal_hypotheses_and_inlier_counts)."""
    O = _O()
    Ns, B = 240, 96
    C, CalM, _, _, _ = RC.rig_batch("parallel", 1, Ns, 0.0, seed=11, K="shared")
    scene = C[0].copy()
    rng = np.random.default_rng(3)
    bad = rng.choice(Ns, Ns // 4, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    idx = np.stack([rng.choice(Ns, n, replace=False) for _ in range(B)]).astype(np.int32)
    hyp = gpu_ctx.pose_sampled(method, scene, CalM, idx)
    torch.cuda.synchronize()
    hyp = {k: _np(v) for k, v in hyp.items() if k != "_raw"}
    assert np.all(hyp["status"] == 0)
    ties, worst, control = 0, 0.0, np.inf
    for b in range(0, B, 6):
        Cb = scene[idx[b]].T.copy()
        ob = {k: hyp[k][b] for k in ("T", "R_t_2", "R_t_3")}
        e0, eb = pose_err_any_convention(ob, getattr(O, method), Cb, CalM)
        assert eb < 1e-6, (method, b, e0, eb)
        ties += e0 >= 1e-6
        worst = max(worst, eb)
        control = min(control, pose_err_any_convention(ob, getattr(O, method), Cb, RC.swap_views_23(CalM))[1])
    assert ties <= 2 and control > 1e-3, (method, ties, control)
    _report("c.sampled.%s.route%d" % (method, gpu_ctx.route), worst=worst, control=control)


# ---- d. counts, masks, MSAC --------------------------------------------------------------------------------------------------------------------------------
THR = 4.0


@functools.lru_cache(maxsize=None)
def _score_case():
    """one per-view-K scene of 130 matches (parallel rig, 0.5 px) with a quarter displaced; nine hypotheses, the truth and perturbations of it as in
    tests/test_emulated_score.py; the numpy reference in double: cameras K_v [R|t] with the K of each view, the oracle's triangulation, residuals, the
    rule of experiments_real.m:94-98 -> (scene, CalM, R2 (9,3,4), R3, inlier flags (9,130), F (9,), smallest distance of a residual from the threshold)"""
    O = _O()
    n, B = 130, 9
    Cs, CalM, Rt2, Rt3, _ = RC.rig_batch("parallel", 1, n, 0.5, seed=4, K="shared")
    Rt2, Rt3 = RC.unit_t2(Rt2, Rt3)
    scene = np.ascontiguousarray(Cs[0]).copy()
    rng = np.random.default_rng(104)
    bad = rng.choice(n, n // 4, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    R2 = np.zeros((B, 3, 4)); R3 = np.zeros((B, 3, 4))
    for b in range(B):
        e = rng.normal(0, (0.0, 2e-4, 5e-4, 1e-3)[b % 4], (2, 3, 4))
        R2[b] = Rt2 + e[0]; R3[b] = Rt3 + e[1]
    flags, F, margin = _numpy_scores(O, scene, CalM, R2, R3)
    return scene, CalM, R2, R3, flags, F, margin


def _numpy_scores(O, scene, CalM, R2, R3):
    B, n = R2.shape[0], scene.shape[0]
    flags = np.zeros((B, n), dtype=bool); F = np.zeros(B); margin = np.inf
    for b in range(B):
        Ps = [CalM[0:3] @ np.eye(3, 4), CalM[3:6] @ R2[b], CalM[6:9] @ R3[b]]
        X = O.triangulation3D(Ps, scene.T.copy()); X = X[0:3] / X[3:4]
        res = O.project3Dpoints(X, Ps) - scene.T                              # 6 x n
        flags[b] = np.all(np.abs(res) <= THR, axis=0)
        margin = min(margin, np.abs(np.abs(res) - THR).min())
        ss = np.sum(res * res, axis=0)
        F[b] = (1.0 + 63.0 * (1.0 - ss[flags[b]] / (6.0 * THR * THR))).sum()
    return flags, F, margin


def test_counts_masks_and_msac_scores_with_per_view_calibration(ctx):
    """inlier_count (count and MSAC score, four hypotheses per wavefront and one) and inlier_mask against numpy: no reference residual lies within 1e-6 of
    the threshold, so counts and flags are equal exactly; the score sits in the bracket of tests/test_emulated_score.py, F - count - 1 <= score <= F + 1.
    Control: with K2 and K3 exchanged the reference count of the true pose drops."""
    O = _O()
    scene, CalM, R2, R3, flags, F, margin = _score_case()
    cnt = flags.sum(axis=1)
    assert margin > 1e-6 and cnt[0] >= 90
    assert _numpy_scores(O, scene, RC.swap_views_23(CalM), R2[:1], R3[:1])[0].sum() < cnt[0]
    try:
        for rows in (1, 0):
            ctx.set_count_rows(rows)
            ctx.set_score("count")
            got = _np(ctx.inlier_count(scene, CalM, R2, R3, THR))
            assert np.array_equal(got, cnt), (rows, got.tolist(), cnt.tolist())
            mask, mc = ctx.inlier_mask(scene, CalM, R2, R3, THR, with_counts=True)
            assert np.array_equal(_np(mask) != 0, flags) and np.array_equal(_np(mc), cnt), rows
            ctx.set_score("msac")
            soft = _np(ctx.inlier_count(scene, CalM, R2, R3, THR)).astype(np.int64)
            assert (F - cnt - 1 <= soft).all() and (soft <= F + 1).all(), (rows, soft.tolist(), F.tolist())
    finally:
        ctx.set_score("count"); ctx.set_count_rows(1)


def test_rt_from_tft_with_per_view_calibration(ctx):
    O = _O()
    B, N = 9, 30
    worst, control = 0.0, np.inf
    for rig in ("roll", "forward"):
        C, CalM, _, _, _ = RC.rig_batch(rig, B, N, 0.5, seed=55, K="shared")
        T = np.stack([O.LinearTFTPoseEstimation(C[b].T.copy(), CalM)[3] for b in range(B)])
        R2, R3, st = ctx.rt_from_tft(T, CalM, C)
        R2, R3, st = _np(R2), _np(R3), _np(st)
        assert np.all(st == 0)
        for b in range(B):
            o2, o3 = O.R_t_from_TFT(T[b], CalM, C[b].T.copy())
            s2, s3 = O.R_t_from_TFT(T[b], RC.swap_views_23(CalM), C[b].T.copy())
            worst = max(worst, rel_err(R2[b], o2), rel_err(R3[b], o3))
            control = min(control, max(rel_err(R2[b], s2), rel_err(R3[b], s3)))
    assert worst < TOL_LINEAR and control > 1e-3, (worst, control)
    _report("d.rt_from_tft", worst=worst, control=control)


# ---- e. robust estimators ------------------------------------------------------------------------------------------------------------------------------------
def _robust_scenes():
    """three scenes of 17, 60 and 130 exact matches (rigs roll, parallel, converging), a quarter of each displaced by 20 .. 80 px in views 2 and 3,
    calibrated by per_view_K(0), (1), (2) -> (items, CalM (3, 9, 3), clean flags per scene)"""
    sizes, rigs = [17, 60, 130], ["roll", "parallel", "converging"]
    CalM = RC.per_view_calm(3)
    items, clean = [], []
    rng = np.random.default_rng(9)
    for s, n in enumerate(sizes):
        scene = RC.rig_batch(rigs[s], 1, n, 0.0, seed=600 + s, K=CalM[s])[0][0].copy()
        bad = rng.choice(n, n // 4, replace=False)
        scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4)) * rng.choice([-1.0, 1.0], size=(bad.size, 4))
        ok = np.ones(n, dtype=bool); ok[bad] = False
        items.append(scene); clean.append(ok)
    return items, CalM, clean


def _bits(a):
    return np.ascontiguousarray(_np(a), dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("score", ["count", "msac"])
@pytest.mark.parametrize("method", LINEAR)
def test_robust_scenes_with_a_calibration_per_scene(ctx, method, score):
    """robust_pose_scenes with calm (S, 9, 3): scene s is bit for bit what robust_pose returns for it alone with its own CalM and seed + s (the documented
    contract; it holds only if scene s reads calm + 27 s); robust_pose is the composition of the public pieces (test_gpu_robust._definition, count
    ranking); and the returned mask is exactly the uncorrupted matches."""
    from tft_vs_fund_amd import api
    from test_gpu_robust import _definition, _assert_equal
    items, CalM, clean = _robust_scenes()
    packed, off = api.pack_ragged(items)
    n_hyp, thr, seed = 256, 1.0, 77
    try:
        ctx.set_score(score)
        out = ctx.robust_pose_scenes(method, _dev(packed), _dev(off), _dev(CalM), n_hyp, thr, seed=seed)
        torch.cuda.synchronize()
        out = {k: _np(v) for k, v in out.items()}
        for s, scene in enumerate(items):
            one = ctx.robust_pose(method, _dev(scene), _dev(CalM[s]), n_hyp, thr, seed=seed + s)
            torch.cuda.synchronize()
            assert int(one["status"]) == 0 and int(out["status"][s]) == 0, (method, score, s)
            for k in ("R_t_2", "R_t_3", "T"):
                assert np.array_equal(_bits(out[k][s]), _bits(one[k])), (method, score, s, k)
            for k in ("inliers", "hypothesis", "refits", "candidates") + (("score",) if score == "msac" else ()):
                assert int(out[k][s]) == int(one[k]), (method, score, s, k)
            m = out["mask"][off[s]:off[s + 1]]
            assert np.array_equal(m, _np(one["mask"])), (method, score, s)
            assert np.array_equal(m != 0, clean[s]), (method, score, s, int(m.sum()), int(clean[s].sum()))
            if score == "count":
                _assert_equal(one, _definition(ctx, method, scene, CalM[s], n_hyp, thr, seed=seed + s), (method, s))
    finally:
        ctx.set_score("count")


def test_robust_refine_and_polish_hand_the_calibration_on(ctx):
    """refine="OptimFPoseEstimation" and polish=True, the two places where robust_pose_scenes hands CalM (S, 9, 3) to a second kernel family: each equals
    that second step called by hand on the scene's inliers with the scene's own CalM."""
    from tft_vs_fund_amd import api
    items, CalM, clean = _robust_scenes()
    packed, off = api.pack_ragged(items)
    out = ctx.robust_pose_scenes("LinearTFTPoseEstimation", _dev(packed), _dev(off), _dev(CalM), 256, 1.0, seed=77, refine="OptimFPoseEstimation", polish=True)
    torch.cuda.synchronize()
    out = {k: _np(v) for k, v in out.items()}
    O = _O()
    for s, scene in enumerate(items):
        m = out["mask"][off[s]:off[s + 1]] != 0
        assert int(out["status"][s]) == 0 and np.array_equal(m, clean[s])
        inl = np.ascontiguousarray(scene[m])
        ref = _pose(ctx, "OptimFPoseEstimation", inl[None], CalM[s], reconst=False)
        assert int(out["status_refined"][s]) == 0 and int(out["iter_refined"][s]) == int(ref["iter"][0])
        for k in ("R_t_2", "R_t_3", "T"):
            assert np.array_equal(_bits(out[k + "_refined"][s]), _bits(ref[k][0])), (s, k)
        o = O.OptimFPoseEstimation(inl.T.copy(), CalM[s])                    # (and that step is the oracle's with the scene's calibration)
        assert max(rel_err(ref["R_t_2"][0], o[0]), rel_err(ref["R_t_3"][0], o[1])) < TOL_OPTIMF
        ba = ctx.bundle_adjust(CalM[s], out["R_t_2"][s][None], out["R_t_3"][s][None], inl[None])
        torch.cuda.synchronize()
        assert int(out["status_polished"][s]) == 0 and int(out["iter_polished"][s]) == int(ba["iter"][0])
        assert np.array_equal(_bits(out["R_t_2_polished"][s]), _bits(ba["R_t_2"][0])) and np.array_equal(_bits(out["R_t_3_polished"][s]), _bits(ba["R_t_3"][0]))
        assert np.array_equal(_bits(out["repr_err_polished"][s]), _bits(ba["repr_err"][0]))


# ---- f. BundleAdjustment -----------------------------------------------------------------------------------------------------------------------------------
def _perturbed(R_t, rng):
    """poses near the truth, as tests/test_bundle_adjustment.py::_views_case: ~0.5 degrees, 1 % on the translations; the first camera stays"""
    R0 = R_t.copy()
    for j in range(1, R_t.shape[0] // 3):
        w = 0.01 * rng.standard_normal(3); th = np.linalg.norm(w); k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R0[3 * j:3 * j + 3, :3] = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx) @ R_t[3 * j:3 * j + 3, :3]
        R0[3 * j:3 * j + 3, 3] = R_t[3 * j:3 * j + 3, 3] * (1 + 0.01 * rng.standard_normal(3))
    return R0


def _ba_items(sizes, K):
    """one three-view problem per size, rigs in turn, noise 1 px -> (C list of (n, 6), CalM, R0 (B, 9, 4) start poses)"""
    rigs = ["converging", "roll", "forward", "parallel", "collinear_parallel"]
    B = len(sizes)
    CalM = RC.per_view_calm(B) if K == "per_view" else RC.per_view_calm()
    rng = np.random.default_rng(12)
    Cs, R0 = [], []
    for b, n in enumerate(sizes):
        C, _, Rt2, Rt3, _ = RC.rig_batch(rigs[b % 5], 1, n, 1.0, seed=700 + b, K=RC.calm_item(CalM, b))
        Rt2, Rt3 = RC.unit_t2(Rt2, Rt3)
        Cs.append(C[0]); R0.append(_perturbed(np.vstack([np.eye(3, 4), Rt2, Rt3]), rng))
    return Cs, CalM, np.stack(R0)


def _check_ba(got2, got3, rec, it, err, ref, swapped, what):
    Ro, Xo, ito, erro = ref
    assert int(it) == ito, (what, int(it), ito)
    e = max(rel_err(got2, Ro[3:6]), rel_err(got3, Ro[6:9]), rel_err(rec, Xo), abs(float(err) - erro) / erro)
    assert e < TOL_BA, (what, e)
    d = max(rel_err(got2, swapped[0][3:6]), rel_err(got3, swapped[0][6:9]))
    assert d > 1e-3, (what, d)
    return e, d


@pytest.mark.parametrize("K", ["per_view", "shared"])
def test_bundle_adjust_with_per_view_calibration(ctx, K):
    from oracle import ba_oracle as BA
    N = 33
    Cs, CalM, R0 = _ba_items([N] * 5, K)
    out = ctx.bundle_adjust(CalM, R0[:, 3:6], R0[:, 6:9], np.stack(Cs))
    torch.cuda.synchronize()
    out = {k: _np(v) for k, v in out.items()}
    assert np.all(out["status"] == 0)
    worst, control = 0.0, np.inf
    for b in range(5):
        Kb = RC.calm_item(CalM, b)
        ref = BA.BundleAdjustment(Kb, R0[b], Cs[b].T.copy(), None)
        sw = BA.BundleAdjustment(RC.swap_views_23(Kb), R0[b], Cs[b].T.copy(), None)
        e, d = _check_ba(out["R_t_2"][b], out["R_t_3"][b], out["Reconst"][b], out["iter"][b], out["repr_err"][b], ref, sw, (K, b))
        worst, control = max(worst, e), min(control, d)
    _report("f.bundle_adjust.%s" % K, worst=worst, control=control)


def test_bundle_adjust_ragged_with_a_calibration_per_item(ctx):
    """n = 12, 33, 90 in one call, a mask that drops every fifth correspondence, CalM (B, 9, 3): the oracle on each item's selected correspondences"""
    from oracle import ba_oracle as BA
    from tft_vs_fund_amd import api
    sizes = [12, 33, 90, 33, 12]
    Cs, CalM, R0 = _ba_items(sizes, "per_view")
    packed, off = api.pack_ragged(Cs)
    mask = np.ones(packed.shape[0], dtype=np.uint8)
    for b, n in enumerate(sizes):
        if n > 12:
            mask[off[b] + 2:off[b + 1]:5] = 0
    out = ctx.bundle_adjust_ragged(_dev(CalM), _dev(R0[:, 3:6]), _dev(R0[:, 6:9]), _dev(packed), _dev(off), mask=_dev(mask))
    torch.cuda.synchronize()
    out = {k: _np(v) for k, v in out.items()}
    assert np.all(out["status"] == 0)
    worst, control = 0.0, np.inf
    for b in range(len(sizes)):
        sel = mask[off[b]:off[b + 1]] != 0
        assert int(out["used"][b]) == int(sel.sum())
        Cb = Cs[b][sel].T.copy()
        ref = BA.BundleAdjustment(CalM[b], R0[b], Cb, None)
        sw = BA.BundleAdjustment(RC.swap_views_23(CalM[b]), R0[b], Cb, None)
        rec = out["Reconst"][off[b]:off[b + 1]]
        assert np.all(np.isnan(rec[~sel]))
        e, d = _check_ba(out["R_t_2"][b], out["R_t_3"][b], rec[sel].T, out["iter"][b], out["repr_err"][b], ref, sw, b)
        worst, control = max(worst, e), min(control, d)
    _report("f.bundle_adjust_ragged", worst=worst, control=control)


@pytest.mark.parametrize("M", [3, 4])
def test_bundle_adjust_views_with_a_calibration_per_view(ctx, M):
    """bundle_adjust_views with M different K (the hand index calm[(3 v + r) + 3 M c] of csrc/ba_views_kernel.h), shared (3M, 3) and per problem
    (B, 3M, 3): the generator's M-view scene re-projected through per-view calibrations."""
    from oracle import ba_oracle as BA
    from tft_vs_fund_amd.scenes import generate_multiview_scene
    B, N = 3, 30
    rng = np.random.default_rng(40 + M)
    worst, control = 0.0, np.inf
    Cs, Ks, R0s = [], [], []
    for b in range(B):
        _, _, R_t, X = generate_multiview_scene(M, N, noise=0.0, seed=50 + b)     # ground-truth poses and points (frame of camera 1)
        Kv = RC.per_view_K(b) + [0.9 * RC.per_view_K(b + 3)[0]]
        CalM = np.vstack(Kv[:M])
        C = np.zeros((2 * M, N))
        for v in range(M):
            xh = CalM[3 * v:3 * v + 3] @ (R_t[3 * v:3 * v + 3, :3] @ X + R_t[3 * v:3 * v + 3, 3:4])
            C[2 * v:2 * v + 2] = xh[0:2] / xh[2:3] + rng.standard_normal((2, N))
        sc = np.linalg.norm(R_t[3:6, 3]); R_t = R_t.copy(); R_t[:, 3] /= sc
        Cs.append(C); Ks.append(CalM); R0s.append(_perturbed(R_t, rng))
    for form in ("per_item", "shared"):
        calm = np.stack(Ks) if form == "per_item" else Ks[0]
        Cf = Cs if form == "per_item" else [Cs[0]] * B
        R0f = R0s if form == "per_item" else [R0s[0], R0s[0], R0s[0]]
        out = ctx.bundle_adjust_views(calm, np.stack(R0f), np.stack([np.ascontiguousarray(c.T) for c in Cf]), None)
        torch.cuda.synchronize()
        out = {k: _np(v) for k, v in out.items()}
        assert np.all(out["status"] == 0)
        for b in range(B if form == "per_item" else 1):
            Kb = Ks[b]
            Ro, Xo, ito, erro = BA.BundleAdjustment(Kb, R0f[b], Cf[b], None)
            assert int(out["iter"][b]) == ito, (M, form, b)
            e = max(rel_err(out["R_t"][b], Ro), rel_err(out["Reconst"][b], Xo), abs(float(out["repr_err"][b]) - erro) / erro)
            assert e < TOL_BA, (M, form, b, e)
            Ksw = Kb.copy(); Ksw[3:6] = Kb[3 * M - 3:3 * M]; Ksw[3 * M - 3:3 * M] = Kb[3:6]      # view 2 <-> the last view
            d = rel_err(out["R_t"][b], BA.BundleAdjustment(Ksw, R0f[b], Cf[b], None)[0])
            assert d > 1e-3, (M, form, b, d)
            worst, control = max(worst, e), min(control, d)
    _report("f.bundle_adjust_views.M%d" % M, worst=worst, control=control)


# ---- g. N across the 4096 switch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [0.0, 1.0])
@pytest.mark.parametrize("N", [4096, 4097])
@pytest.mark.parametrize("method", LINEAR)
def test_votes_on_both_sides_of_n_4096(gpu_ctx, method, N, noise):
    """pose_common.h::recover_vote packs the two scores of a call into 16-bit halves up to N = 4096 (|score| = 2 N = 8192 is the extreme the packing has
    to hold) and takes two single passes above.  B = 5, the generator's shared K.  With exact data every vote is unanimous: the scores are +-2 N."""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    O = _O()
    B = 5
    C, CalM, _, _ = generate_scene_batch(B, N, noise=noise, seed=N)
    out = _pose(gpu_ctx, method, C, CalM)
    votes = _pose(gpu_ctx, method, C, CalM, debug=True)["debug"][:, 60:68]
    assert np.all(out["status"] == 0)
    worst = 0.0
    for b in range(B):
        R2, R3, Rec, T, _ = getattr(O, method)(C[b].T.copy(), CalM)
        e = max(rel_err_T(out["T"][b], T), rel_err(out["R_t_2"][b], R2), rel_err(out["R_t_3"][b], R3), rel_err(out["Reconst"][b], Rec))
        assert e < TOL_LINEAR, (method, N, noise, b, e)
        worst = max(worst, e)
        if noise == 0.0:
            for v in (votes[b, 0:4], votes[b, 4:8]):
                assert sorted(np.abs(v).tolist()) == [0.0, 0.0, 2.0 * N, 2.0 * N] or np.abs(v).tolist() == [2.0 * N] * 4, (method, N, b, v.tolist())
                assert v.max() == 2.0 * N
    _report("g.%s.N%d.noise%g.route%d" % (method, N, noise, gpu_ctx.route), worst=worst)


# ---- h. host entry points -----------------------------------------------------------------------------------------------------------------------------------
def test_host_entry_points_equal_their_device_twins(ctx):
    """numpy in -> the _host forms of the C ABI, which copy CalM themselves: pose_batch with (B, 9, 3), pose_batch_ragged and bundle_adjust_ragged on host
    arrays, each equal to the device path bit for bit."""
    from tft_vs_fund_amd import api
    B, N = 9, 20
    C, CalM, _, _, _ = RC.rig_batch("roll", B, N, 0.5, seed=81, K="per_view")
    for method in LINEAR + ["OptimFPoseEstimation", "ResslTFTPoseEstimation"]:
        host = ctx.pose_batch(method, C, CalM, reconst=True)
        dev = _pose(ctx, method, C, CalM)
        for k in ("T", "R_t_2", "R_t_3", "Reconst", "iter", "status"):
            assert np.array_equal(np.asarray(host[k]), dev[k]), (method, k)
    sizes = [8, 49, 12, 201, 12]
    CalM = RC.per_view_calm(len(sizes))
    items = [RC.rig_batch("forward", 1, n, 0.5, seed=90 + b, K=CalM[b])[0][0] for b, n in enumerate(sizes)]
    packed, off = api.pack_ragged(items)
    for method in LINEAR + ["OptimFPoseEstimation"]:
        host = ctx.pose_batch_ragged(method, packed, off, CalM, reconst=True)
        dev = ctx.pose_batch_ragged(method, _dev(packed), _dev(off), _dev(CalM), reconst=True)
        torch.cuda.synchronize()
        for k in ("T", "R_t_2", "R_t_3", "Reconst", "iter", "status"):
            assert np.array_equal(np.asarray(host[k]), _np(dev[k])), (method, k)
    Cs, CalM, R0 = _ba_items([12, 33, 90], "per_view")
    packed, off = api.pack_ragged(Cs)
    mask = np.ones(packed.shape[0], dtype=np.uint8); mask[5::7] = 0
    host = ctx.bundle_adjust_ragged(CalM, R0[:, 3:6], R0[:, 6:9], packed, off, mask=mask)
    dev = ctx.bundle_adjust_ragged(_dev(CalM), _dev(R0[:, 3:6]), _dev(R0[:, 6:9]), _dev(packed), _dev(off), mask=_dev(mask))
    torch.cuda.synchronize()
    assert np.all(host["status"] == 0)
    for k in ("R_t_2", "R_t_3", "Reconst", "iter", "repr_err", "used", "status"):
        assert np.array_equal(np.asarray(host[k]), _np(dev[k]), equal_nan=True), k
