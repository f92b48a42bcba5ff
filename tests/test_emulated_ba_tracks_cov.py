"""
The covariance kernel of the bundle adjustment over tracks (csrc/ba_tracks_cov_kernel.h: k_ba_tracks_cov<M, none | Huber | Cauchy>) on the lane
emulator, no GPU, compiled by g++ (tests/emu/emu_ba_tracks_cov.cpp), against the numpy restatement (tests/ba_tracks_cov_oracle.py: the dense bordered
inverse) over the cases of tests/ba_tracks_cov_cases.py for M = 3 and 6.  The kernel is evaluated at the restatement's own final parameters, so both
sides see the same x.  Gate (ba_tracks_cov_cases.gate): cov and every point block within 1e-9 of the block's largest entry, sigma0 within 1e-9, cov
symmetric to the bit, |cov h_P| <= 1e-9 |cov|, an unseen camera's rows exactly 0, NaN exactly over the dropped points.  Appended all-NaN columns change
no bit; an item without a covariance gives NaN.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ba_tracks_cov_cases as tcc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i, c_d = ctypes.c_long, ctypes.c_int, ctypes.c_double
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
EMU_VIEWS = (3, 6)


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_ba_tracks_cov.so")
    deps = [os.path.join(emu, f) for f in ("emu_ba_tracks_cov.cpp", "emu_primitives.h", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_ba_tracks_cov.cpp")], check=True)
    return ctypes.CDLL(out)


def run(L, CalM, R_t, C, X, loss, c, points=True):
    """the emulated call, B = 1: CalM 3M x 3, R_t 3M x 4, C 2M x N, X 3 x N -> cov (P, P), sigma0, point_cov (N, 6) or None"""
    M, N = C.shape[0] // 2, C.shape[1]
    Pn = 6 * (M - 1)
    calm = np.ascontiguousarray(CalM.T).reshape(-1); rt = np.ascontiguousarray(R_t.T).reshape(-1)     # (named: a pointer does not keep its array alive)
    Cc = np.ascontiguousarray(C.T); Xc = np.ascontiguousarray(X.T)
    cov, s0, pc = np.full((Pn, Pn), 5.0), np.full(1, 5.0), np.full((N, 6), 5.0) if points else None
    assert L.e_ba_tracks_cov(M, P(calm), c_l(0), P(rt), P(Cc), c_l(1), c_i(N), P(Xc), c_i(tcc.LOSS_ID[loss]), c_d(c or 0.0), P(cov), P(s0), P(pc)) == 0
    return cov, float(s0[0]), pc


@pytest.mark.parametrize("M,N,pattern,loss,c", [k for k in tcc.CASES if k[0] in EMU_VIEWS])
def test_kernel_matches_the_restatement(M, N, pattern, loss, c):
    CalM, _, C, _ = tcc.inputs(M, N, pattern, loss)
    R_t, X = tcc.optimum(M, N, pattern, loss, c)
    cov, s0, pc = run(_lib(), CalM, R_t, C, X, loss, c)
    tcc.gate(tcc.reference(M, N, pattern, loss, c), cov, s0, pc, (M, N, pattern, loss, c), full=(M, N, pattern, loss, c) not in tcc.LEFT_OUT)


@pytest.mark.parametrize("M", EMU_VIEWS)
@pytest.mark.parametrize("loss,c", tcc.LOSSES[0:3:2])
def test_appended_nan_columns_change_no_bit_and_point_cov_is_an_output_only(M, loss, c):
    """the padding that serves as the ragged form of this call: N = 65 padded to 130 equals N = 65"""
    L = _lib()
    CalM, _, C, _ = tcc.inputs(M, 65, "random", loss)
    R_t, X = tcc.optimum(M, 65, "random", loss, c)
    cov, s0, pc = run(L, CalM, R_t, C, X, loss, c)
    Cp, Xp = tcc.padded(C, X)
    cov2, s02, pc2 = run(L, CalM, R_t, Cp.T, Xp.T, loss, c)
    assert tcc.biteq(cov, cov2) and s0 == s02 and tcc.biteq(pc, pc2[:65]) and np.isnan(pc2[65:]).all()
    cov3, s03, _ = run(L, CalM, R_t, C, X, loss, c, points=False)
    assert tcc.biteq(cov, cov3) and s0 == s03


@pytest.mark.parametrize("loss,c", tcc.LOSSES[0:2])
def test_a_moved_frame_and_any_scale_give_the_covariance_in_the_output_frame(loss, c):
    """poses and points in a frame whose first camera is not [I|0] and in a common scale of 2.5: the same definition evaluated after the kernel's change
    of coordinates, so the same 1e-9"""
    M, N, pattern = 4, 65, "random"
    CalM, _, C, _ = tcc.inputs(M, N, pattern, loss)
    R_t, X = tcc.optimum(M, N, pattern, loss, c)
    a = 0.3
    G = np.eye(4); G[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]; G[:3, 3] = [0.2, -0.1, 0.4]
    Rm = np.vstack([R_t[3 * j:3 * j + 3] @ G for j in range(M)])
    ok = ~np.isnan(X).all(axis=0)
    Xm = X.copy(); Xm[:, ok] = (np.linalg.inv(G) @ np.vstack([X[:, ok], np.ones(int(ok.sum()))]))[:3]
    Rm[:, 3] *= 2.5; Xm = 2.5 * Xm
    cov, s0, pc = run(_lib(), CalM, Rm, C, Xm, loss, c)
    tcc.gate(tcc.reference(M, N, pattern, loss, c), cov, s0, pc, (M, N, pattern, loss, c, "moved, scale 2.5"))


@pytest.mark.parametrize("kind", tcc.FAILING)
@pytest.mark.parametrize("loss,c", tcc.LOSSES[0:2])
def test_items_without_a_covariance_give_nan(kind, loss, c):
    M, CalM, R_t, C, X = tcc.failing(kind)
    ref = tcc.TCO.covariance(CalM, R_t, C, X, loss, c)
    assert np.isnan(ref["cov"]).all() and np.isnan(ref["sigma0"]) and np.isnan(ref["point_cov"]).all()
    cov, s0, pc = run(_lib(), CalM, R_t, C, X, loss, c)
    assert np.isnan(cov).all() and np.isnan(s0) and np.isnan(pc).all()


def test_a_nan_point_taking_part_gives_nan_and_no_further_instance():
    L = _lib()
    CalM, _, C, _ = tcc.inputs(3, 12, "full", None)
    R_t, X = tcc.optimum(3, 12, "full", None, None)
    X = X.copy(); X[1, 5] = np.inf
    cov, s0, pc = run(L, CalM, R_t, C, X, None, None)
    assert np.isnan(cov).all() and np.isnan(s0) and np.isnan(pc).all()
    assert L.e_ba_tracks_cov(7, *([None] * 3), None, c_l(1), c_i(12), None, c_i(0), c_d(0.0), None, None, None) == -1
    assert L.e_ba_tracks_cov(3, *([None] * 3), None, c_l(1), c_i(12), None, c_i(3), c_d(1.0), None, None, None) == -1
