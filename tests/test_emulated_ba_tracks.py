"""
The bundle adjustment over tracks (csrc/ba_tracks_kernel.h: k_bundle_adjust_tracks<2 .. 6>, per-point visibility) on the lane emulator, no GPU, compiled
by g++ (tests/emu/emu_ba_tracks.cpp), against the numpy restatement (tests/ba_tracks_oracle.py) over every case of tests/ba_tracks_cases.py at its gates:
status and used exact, iter equal, repr_err, R_t and the Reconst columns of the points taking part within 1e-9 relative, NaN exactly at the dropped
columns.  The restatement itself is pinned by finite differences and by MINPACK at the converged optimum of a partially visible case.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ba_tracks_cases as tc
import ba_tracks_oracle as TO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i = ctypes.c_long, ctypes.c_int
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_ba_tracks.so")
    deps = [os.path.join(emu, f) for f in ("emu_ba_tracks.cpp", "emu_primitives.h", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_ba_tracks.cpp")], check=True)
    return ctypes.CDLL(out)


def run(L, CalM, R0, C, X0, outputs=True):
    """the emulated call, B = 1 -> (R_t, Reconst, iter, repr_err, used, status)"""
    M, N = C.shape[0] // 2, C.shape[1]
    calm = np.ascontiguousarray(CalM.T).reshape(-1); rt = np.ascontiguousarray(R0.T).reshape(-1); Cc = np.ascontiguousarray(C.T)
    x0 = np.ascontiguousarray(X0.T) if X0 is not None else None
    out = np.full(12 * M, 5.0); rec = np.full((N, 3), 5.0); it = np.full(1, 5, dtype=np.int32); err = np.full(1, 5.0)
    used = np.full(1, -5, dtype=np.int32); st = np.full(1, 5, dtype=np.int32)
    if outputs:
        assert L.e_ba_tracks(M, P(calm), c_l(0), P(rt), P(Cc), c_l(1), c_i(N), P(x0), P(out), P(rec), P(it), P(err), P(used), P(st)) == 0
    else:                                                                                # every output but Rt may be NULL
        assert L.e_ba_tracks(M, P(calm), c_l(0), P(rt), P(Cc), c_l(1), c_i(N), P(x0), P(out), None, None, None, None, None) == 0
    return out.reshape(4, 3 * M).T, rec.T, int(it[0]), float(err[0]), int(used[0]), int(st[0])


@pytest.mark.parametrize("M,N,pattern,with_x0", tc.SYNTHETIC)
def test_kernel_matches_the_restatement(M, N, pattern, with_x0):
    got = run(_lib(), *tc.synthetic(M, N, pattern, with_x0))
    tc.gate(got, tc.reference("syn", M, N, pattern, with_x0), (M, N, pattern, with_x0))


@pytest.mark.parametrize("dataset,first,M,n_tracks", tc.REAL)
def test_kernel_matches_the_restatement_on_epfl_windows(dataset, first, M, n_tracks):
    case = tc.real(dataset, first, M, n_tracks)
    nvis = TO.visibility(case[2]).sum(axis=0)
    assert 60 <= case[2].shape[1] <= 72 and nvis.min() >= 3 and (nvis < M).any()         # real tracks, some of them partial
    ref = tc.reference("real", dataset, first, M, n_tracks)
    assert ref[5] == TO.ST_OK and 1 <= ref[2] <= 30
    tc.gate(run(_lib(), *case), ref, (dataset, first, M))


@pytest.mark.parametrize("kind", tc.FAILING)
def test_failing_items(kind):
    case, used, status = tc.failing(kind)
    ref = tc.reference("fail", kind)
    assert (ref[4], ref[5]) == (used, status)
    tc.gate(run(_lib(), *case), ref, kind)


def test_an_unseen_view_keeps_its_pose_and_null_outputs_change_nothing():
    L = _lib()
    M, N = 4, 65
    CalM, R0, C, X0 = tc.synthetic(M, N, "view_nan", False)
    R_t, X, it, err, used, st = run(L, CalM, R0, C, X0)
    assert st == 0 and used == N
    # in the frame of camera 1 (BundleAdjustment.m:80-86) the camera of the unseen view is where it started, its translation in the output scale 1/|t2|
    G = np.vstack([R0[0:3], [0, 0, 0, 1]])
    start = R0[3 * (M - 1):3 * M] @ np.linalg.inv(G)
    sc = np.linalg.norm(R_t[3 * (M - 1):3 * M, 3]) / np.linalg.norm(start[:, 3])
    assert np.abs(R_t[3 * (M - 1):3 * M, :3] - start[:, :3]).max() < 1e-12 and np.abs(R_t[3 * (M - 1):3 * M, 3] - sc * start[:, 3]).max() < 1e-12
    assert abs(np.linalg.norm(R_t[3:6, 3]) - 1) < 1e-12
    R2 = run(L, CalM, R0, C, X0, outputs=False)[0]
    assert np.array_equal(R2, R_t)
    assert L.e_ba_tracks(7, *([None] * 3), None, c_l(1), c_i(N), *([None] * 7)) == -1    # no seventh instance


@pytest.mark.parametrize("N0,N1", [(64, 65), (65, 130)])
def test_appended_nan_columns_change_no_bit(N0, N1):
    """the padding that serves as the ragged form of this call"""
    L = _lib()
    for M, pattern, with_x0 in ((3, "random", False), (6, "few_obs", True)):
        CalM, R0, C, X0 = tc.synthetic(M, N0, pattern, with_x0)
        a = run(L, CalM, R0, C, X0)
        Cp = np.hstack([C, np.full((2 * M, N1 - N0), np.nan)])
        Xp = np.hstack([X0, np.full((3, N1 - N0), 7.0)]) if with_x0 else None
        b = run(L, CalM, R0, Cp, Xp)
        assert a[2:] == b[2:] and a[0].tobytes() == b[0].tobytes()
        assert a[1].tobytes() == np.ascontiguousarray(b[1][:, :N0]).tobytes() and np.isnan(b[1][:, N0:]).all()


def test_restatement_jacobian_and_converged_optimum():
    worst, dev = TO.check_jacobian_and_optimum(*tc.synthetic(4, 12, "random", False))
    assert worst < 1e-7 and dev < 1e-5
    worst, dev = TO.check_jacobian_and_optimum(*tc.synthetic(3, 12, "one_missing", True))
    assert worst < 1e-7 and dev < 1e-5


def test_restatement_on_full_visibility_is_the_reference_as_restated():
    from oracle import ba_oracle as BA
    for with_x0 in (False, True):
        case = tc.synthetic(4, 12, "full", with_x0)
        R_t, X, it, err, used, st = TO.BundleAdjustmentTracks(*case)
        Ro, Xo, ito, erro = BA.BundleAdjustment(*case)
        assert (it, used, st) == (ito, 12, 0) and abs(err - erro) <= 1e-12 * erro and np.abs(R_t - Ro).max() < 1e-12 and np.abs(X - Xo).max() < 1e-12 * np.abs(Xo).max()
