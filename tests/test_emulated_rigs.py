"""
Per-view calibration and unseen camera rigs on the lane emulator, no GPU (tests/rig_cases.py has the cases; tests/test_gpu_rigs.py is the gate on the
device and covers the API, the dispatch of capi.hip, the block kernels and the robust drivers, none of which the emulator has).

Every other input of the suite has K1 = K2 = K3, so a kernel that reads the calibration of the wrong view passes it.  Here the three blocks of CalM
differ (focal length, principal point, skew, overall scale) and differ between the items of a batch, and every comparison carries a control: the same
reference computed with K2 and K3 exchanged must be far from the kernel's result (rig_cases.check_pose_batch).
"""
import ctypes

import numpy as np
import pytest

from oracle import ba_oracle as BA
from oracle import tft_oracle as O
from helpers import rel_err
from emu import emu_build
import rig_cases as RC
from test_emulated_score import _lib as score_lib, _cm, _numpy as score_numpy, _one as score_one, B as N_HYP

TOL_LINEAR = 1e-9          # TOL of tests/test_gpu_rows.py and tests/test_gpu_blocks.py
TOL_OPTIMF = 1e-8          # tests/test_emulated_kernels.py::test_optim_f_kernel_matches_golden
TOL_BA = 1e-9              # the BundleAdjustment gate of the README


@pytest.fixture(scope="module")
def emu():
    return emu_build.load()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def calm_abi(CalM):
    """(9, 3) or (B, 9, 3) -> (column-major doubles, stride) as the C ABI takes them"""
    CalM = np.asarray(CalM, dtype=np.float64)
    if CalM.ndim == 2:
        return np.ascontiguousarray(CalM.T).reshape(-1), 0
    return np.ascontiguousarray(CalM.transpose(0, 2, 1)).reshape(-1), CalM.shape[1] * 3


def run_pose(lib, entry, C, CalM, reconst=True):
    B, N, _ = C.shape
    calm, stride = calm_abi(CalM)
    Rt2 = np.zeros((B, 12)); Rt3 = np.zeros((B, 12)); T = np.zeros((B, 27))
    Rec = np.zeros((B, N, 3)) if reconst else None
    it = np.zeros(B, dtype=np.int32); st = np.zeros(B, dtype=np.int32); dbg = np.zeros((B, 128))
    getattr(lib, entry)(_p(C), _p(calm), ctypes.c_long(stride), ctypes.c_long(B), ctypes.c_int(N), ctypes.c_int(0),
                        _p(Rt2), _p(Rt3), _p(T), _p(Rec), _p(it), _p(st), _p(dbg))
    return dict(R_t_2=Rt2.reshape(B, 4, 3).transpose(0, 2, 1), R_t_3=Rt3.reshape(B, 4, 3).transpose(0, 2, 1),
                T=T.reshape(B, 3, 3, 3).transpose(0, 3, 2, 1), Reconst=None if Rec is None else Rec.transpose(0, 2, 1),
                iter=it, status=st, debug=dbg)


def _entries(method, N):
    """(wave route, rows route) of a method at N correspondences, as capi.hip picks them"""
    if method == "LinearTFTPoseEstimation":
        return ["emu_linear_tft_pose", "emu_linear_tft_pose_rows_exact" if N < 12 else "emu_linear_tft_pose_rows"]
    if method == "LinearFPoseEstimation":
        return ["emu_linear_f_pose", "emu_linear_f_pose_rows_exact" if N < 12 else "emu_linear_f_pose_rows"]
    return ["emu_optim_f_pose", "emu_optim_f_pose_staged"]


# ---- a. linear paths and OptimF ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ["per_view", "shared"])
@pytest.mark.parametrize("rig", RC.RIGS)
@pytest.mark.parametrize("method", ["LinearTFTPoseEstimation", "LinearFPoseEstimation", "OptimFPoseEstimation"])
def test_linear_and_optimf_against_the_oracle(emu, method, rig, K):
    """Five items (a full wavefront of the row kernels and a tail of one), N = the exact tier (linear methods, one CalM per item) and N = 12, noise 0.5 px, both routes."""
    B = 5
    optim = method == "OptimFPoseEstimation"
    tier = 7 if method == "LinearTFTPoseEstimation" else 8
    for N in ((12,) if optim or K == "shared" else (tier, 12)):             # (OptimF's iteration and the exact tiers are slow under emulation)
        tol = TOL_OPTIMF if optim else TOL_LINEAR
        C, CalM, _, _, _ = RC.well_posed_batch(rig, B, N, 0.5, 1000 + N, K, method, tol)
        refs = RC.oracle_refs(method, C, CalM)
        for entry in _entries(method, N):
            out = run_pose(emu, entry, C, CalM)
            votes = None if entry.endswith("staged") else out["debug"][:, 60:68]
            RC.check_pose_batch(out, method, C, CalM, tol, refs, votes=votes, same_iter=optim, what="%s N=%d" % (entry, N))


# ---- b. the Gauss-Helmert trifocal methods: what CalM can and cannot touch --------------------------------------------------------------------------
GH = [("emu_ressl_tft_pose", "parallel"), ("emu_nordberg_tft_pose", "converging"), ("emu_faugpapa_tft_pose", "parallel"), ("emu_pi_pose", "converging"),
      ("emu_picol_pose", "collinear_parallel")]


@pytest.mark.parametrize("entry,rig", GH)
def test_iterative_trifocal_methods_use_calm_after_the_iteration_only(emu, entry, rig):
    B, N = 2, 12
    C, CalM, _, _, _ = RC.well_posed_batch(rig, B, N, 0.5, 77, "per_view", "LinearTFTPoseEstimation", 1e-9)
    out = run_pose(emu, entry, C, CalM)
    same_k = run_pose(emu, entry, C, RC.first_view_only(CalM))
    assert np.all(out["status"] == 0)
    for k in ("T", "iter", "status"):
        assert np.array_equal(out[k], same_k[k]), k                           # CalM enters after the iteration (ResslTFTPoseEstimation.m)
    for b in range(B):
        Cb = C[b].T.copy()
        R2, R3 = O.R_t_from_TFT(out["T"][b], CalM[b], Cb)
        assert rel_err(out["R_t_2"][b], R2) < 1e-9 and rel_err(out["R_t_3"][b], R3) < 1e-9
        assert rel_err(out["Reconst"][b], O._final_reconst(CalM[b], R2, R3, Cb)) < 1e-9
        S2, S3 = O.R_t_from_TFT(out["T"][b], RC.swap_views_23(CalM[b]), Cb)
        assert max(rel_err(out["R_t_2"][b], S2), rel_err(out["R_t_3"][b], S3)) > 1e-3


# ---- d. counts and MSAC scores ---------------------------------------------------------------------------------------------------------------------------
def score_item(n=130, seed=4):
    """one per-view-K scene of the parallel rig with a quarter of its matches displaced, and nine hypotheses: the truth and perturbations of it"""
    Cs, CalM, Rt2, Rt3, _ = RC.rig_batch("parallel", 1, n, 0.5, seed=seed, K="shared")
    Rt2, Rt3 = RC.unit_t2(Rt2, Rt3)
    scene = np.ascontiguousarray(Cs[0]).copy()
    rng = np.random.default_rng(100 + seed)
    bad = rng.choice(n, n // 4, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    h2 = np.zeros((N_HYP, 12)); h3 = np.zeros((N_HYP, 12))
    for b in range(N_HYP):
        e = rng.normal(0, (0.0, 2e-4, 5e-4, 1e-3)[b % 4], (2, 3, 4))
        h2[b] = _cm(Rt2 + e[0]); h3[b] = _cm(Rt3 + e[1])
    return scene, np.ascontiguousarray(CalM), h2, h3


def test_count_kernels_read_the_calibration_of_each_view():
    L = score_lib()
    item = score_item()
    cnt, F = score_numpy(L, item)
    hard = score_one(L, "s_repr", item, 0); soft = score_one(L, "s_repr", item, 1)
    assert np.array_equal(hard, cnt) and hard[0] > 60
    assert (F - cnt - 1 <= soft).all() and (soft <= F + 1).all()
    for fn in ("s_staged", "s_rows"):
        assert np.array_equal(score_one(L, fn, item, 0), hard) and np.array_equal(score_one(L, fn, item, 1), soft), fn
    swapped = (item[0], RC.swap_views_23(item[1]), item[2], item[3])
    assert score_numpy(L, swapped)[0][0] < cnt[0]                            # (the case can see a view mix-up)


# ---- f. BundleAdjustment -----------------------------------------------------------------------------------------------------------------------------------
def ba_case(rig, N, seed, K):
    """one three-view problem near its optimum: the ground truth perturbed as tests/test_bundle_adjustment.py::_views_case does"""
    C, CalM, Rt2, Rt3, _ = RC.rig_batch(rig, 1, N, 1.0, seed=seed, K=K)
    Rt2, Rt3 = RC.unit_t2(Rt2, Rt3)
    rng = np.random.default_rng(seed)
    R0 = np.vstack([np.eye(3, 4), Rt2, Rt3])
    for j in (1, 2):
        w = 0.01 * rng.standard_normal(3); th = np.linalg.norm(w); k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R0[3 * j:3 * j + 3, :3] = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx) @ R0[3 * j:3 * j + 3, :3]
        R0[3 * j:3 * j + 3, 3] *= 1 + 0.01 * rng.standard_normal(3)
    return np.ascontiguousarray(C[0]), (CalM[0] if CalM.ndim == 3 else CalM), R0


def test_bundle_adjustment_kernels_with_per_view_calibration(emu):
    for rig, N in (("converging", 12), ("roll", 33)):
        C, CalM, R0 = ba_case(rig, N, 5 + N, "shared")
        Ro, Xo, ito, erro = BA.BundleAdjustment(CalM, R0, C.T.copy(), None)
        Rs = BA.BundleAdjustment(RC.swap_views_23(CalM), R0, C.T.copy(), None)[0]
        assert rel_err(Rs, Ro) > 1e-3
        calm, _ = calm_abi(CalM)
        r2 = np.ascontiguousarray(R0[3:6].T).reshape(1, 12); r3 = np.ascontiguousarray(R0[6:9].T).reshape(1, 12)
        o2 = np.zeros((1, 12)); o3 = np.zeros((1, 12)); rec = np.zeros((1, N, 3)); it = np.zeros(1, dtype=np.int32); err = np.zeros(1); st = np.zeros(1, dtype=np.int32)
        emu.emu_bundle_adjust(_p(calm), ctypes.c_long(0), _p(r2), _p(r3), _p(C), ctypes.c_long(1), ctypes.c_int(N), None, _p(o2), _p(o3), _p(rec), _p(it), _p(err), _p(st))
        assert st[0] == 0 and it[0] == ito and abs(err[0] - erro) <= TOL_BA * erro
        assert rel_err(o2[0].reshape(4, 3).T, Ro[3:6]) < TOL_BA and rel_err(o3[0].reshape(4, 3).T, Ro[6:9]) < TOL_BA and rel_err(rec[0].T, Xo) < TOL_BA
        rt = np.ascontiguousarray(R0.T).reshape(-1)
        out = np.zeros(36); rec = np.zeros((N, 3))
        assert emu.emu_bundle_adjust_views(3, _p(calm), ctypes.c_long(0), _p(rt), _p(C), ctypes.c_long(1), ctypes.c_int(N), None, _p(out), _p(rec), _p(it), _p(err), _p(st)) == 0
        assert st[0] == 0 and it[0] == ito and abs(err[0] - erro) <= TOL_BA * erro
        assert rel_err(out.reshape(4, 9).T, Ro) < TOL_BA and rel_err(rec.T, Xo) < TOL_BA


# ---- g. N across the switch of recover_vote's packed scores ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,method", [("emu_linear_tft_pose", "LinearTFTPoseEstimation"), ("emu_linear_f_pose_rows", "LinearFPoseEstimation")])
def test_votes_on_both_sides_of_n_4096(emu, entry, method):
    """pose_common.h::recover_vote packs two scores into 16-bit halves up to N = 4096 (|score| = 2 N = 8192 is the packing's extreme) and takes two
    single passes above: exact data, so every vote is unanimous."""
    for N in (4096, 4097):
        C, CalM, _, _, _ = RC.rig_batch("converging", 1, N, 0.0, seed=N, K="generator")
        out = run_pose(emu, entry, C, CalM)
        assert out["status"][0] == 0
        R2, R3, Rec, T, _ = getattr(O, method)(C[0].T.copy(), CalM)
        assert max(rel_err(out["R_t_2"][0], R2), rel_err(out["R_t_3"][0], R3), rel_err(out["Reconst"][0], Rec)) < TOL_LINEAR
        v = out["debug"][0, 60:68]
        assert sorted(np.abs(v[0:4])) == [0, 0, 2 * N, 2 * N] or sorted(np.abs(v[0:4]))[2:] == [2 * N, 2 * N], v
