"""
The covariance kernel of the bundle adjustment (csrc/ba_cov_kernel.h: k_ba_cov, no loss, Huber, Cauchy) on the lane emulator, no GPU, compiled by g++
(tests/emu/emu_ba_cov.cpp), against the numpy restatement (tests/ba_cov_oracle.py: the dense bordered inverse).  The kernel is evaluated at the
restatement's own final parameters, so both sides see the same x: N = 4, 12, 64, 65, 129 with 0, 0, 8, 13, 0 displaced matches, no loss and both
losses at c = 1.5 and 3.  Gates (ba_cov_cases.gate): cov and every point block within 1e-9 of the block's largest entry, sigma0 within 1e-9, cov
symmetric to the bit, |cov h12| <= 1e-9 |cov|.  N = 3 has no redundancy: NaN.  The ragged chain gives every item the bits of the fixed call on its
selection.  The chain has no launch classes -- the kernel's LDS does not grow with N --, so the plan's class bounds, tiny here, change nothing.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ba_cov_cases as cc
import ba_loss_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i, c_d = ctypes.c_long, ctypes.c_int, ctypes.c_double
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_ba_cov.so")
    deps = [os.path.join(emu, f) for f in ("emu_ba_cov.cpp", "emu_primitives.h", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_ba_cov.cpp")], check=True)
    return ctypes.CDLL(out)


def _cm(Rt):
    return np.ascontiguousarray(Rt.T).reshape(12)


def _fixed(L, C, CalM, Rt2, Rt3, X, loss, c, points=True):
    """the emulated fixed-N call, B = 1: C (N, 6), Rt2, Rt3 3x4, X (N, 3) -> cov (144,), sigma0, point_cov (N, 6) or None"""
    N = C.shape[0]
    C = np.ascontiguousarray(C); X = np.ascontiguousarray(X)
    calm, r2, r3 = np.ascontiguousarray(CalM.T).reshape(27), _cm(Rt2), _cm(Rt3)           # (named: a pointer does not keep its array alive)
    cov, s0, pc = np.full(144, 5.0), np.full(1, 5.0), np.full((N, 6), 5.0) if points else None
    assert L.e_ba_cov_fixed(P(calm), c_l(0), P(r2), P(r3), P(C), c_l(1), c_i(N), P(X), c_i(cc.LOSS_ID[loss]), c_d(c or 0.0), P(cov), P(s0), P(pc)) == 0
    return cov, float(s0[0]), pc


@pytest.mark.parametrize("n,n_bad,loss,c", cc.CASES)
def test_kernel_matches_the_restatement(n, n_bad, loss, c):
    L = _lib()
    sc = bc.scene(n, n_bad)
    R_t, X = cc.optimum(n, n_bad, loss, c)
    cov, s0, pc = _fixed(L, sc["C"], sc["CalM"], R_t[3:6], R_t[6:9], X.T, loss, c)
    cc.gate(cc.reference(n, n_bad, loss, c), cov.reshape(12, 12), s0, pc, (n, n_bad, loss, c))
    cov2, s02, _ = _fixed(L, sc["C"], sc["CalM"], R_t[3:6], R_t[6:9], X.T, loss, c, points=False)
    assert cc.biteq(cov, cov2) and s0 == s02                                   # the point blocks are an output and nothing else


@pytest.mark.parametrize("loss,c", cc.LOSSES[0:4:3])
def test_any_scale_of_the_input_gives_the_covariance_at_unit_t2(loss, c):
    """poses and points in a common scale of 2.5: the same definition evaluated another way, so the same 1e-9"""
    L = _lib()
    n, n_bad = 65, 13
    sc = bc.scene(n, n_bad)
    R_t, X = cc.optimum(n, n_bad, loss, c)
    g = np.array([1.0, 1.0, 1.0, 2.5])
    cov, s0, pc = _fixed(L, sc["C"], sc["CalM"], R_t[3:6] * g, R_t[6:9] * g, 2.5 * X.T, loss, c)
    cc.gate(cc.reference(n, n_bad, loss, c), cov.reshape(12, 12), s0, pc, (n, n_bad, loss, c, "scale 2.5"))


@pytest.mark.parametrize("loss,c", cc.LOSSES[0:2])
def test_no_redundancy_and_bad_poses_give_nan(loss, c):
    L = _lib()
    sc = bc.scene(12, 0)
    for C, Rt2, X in ((sc["C"][:3], sc["start"][0], sc["X0"][:3]), (sc["C"], sc["start"][0] * np.nan, sc["X0"])):
        cov, s0, pc = _fixed(L, C, sc["CalM"], Rt2, sc["start"][1], X, loss, c)
        assert np.isnan(cov).all() and np.isnan(s0) and np.isnan(pc).all()
    assert L.e_ba_cov_fixed(*([None] * 8), c_i(3), c_d(1.0), None, None, None) == -1        # no fourth instance


@pytest.mark.parametrize("loss,c", (("huber", 3.0), (None, None)))
def test_ragged_items_equal_the_fixed_call(loss, c):
    L = _lib()
    rc = cc.ragged_case()
    B, nt = len(rc["sizes"]), rc["nt"]
    bounds = np.array([8, 20, 2 ** 31 - 1], dtype=np.int32)
    fixed = lambda b, sel: _fixed(L, rc["scs"][b]["C"][sel], rc["scs"][b]["CalM"], rc["scs"][b]["start"][0], rc["scs"][b]["start"][1], rc["scs"][b]["X0"][sel], loss, c)
    for mk in (rc["mask"], None):
        cov, s0, pc, st = np.full((B, 144), 5.0), np.full(B, 5.0), np.full((nt + 4, 6), 5.0), np.full(B, 0, dtype=np.int32)
        assert L.e_ba_cov_ragged(P(rc["packed"]), P(rc["off"]), c_l(B), c_l(nt), P(mk), P(rc["calms"]), c_l(27), P(rc["r2"]), P(rc["r3"]), P(rc["X"]), P(bounds),
                                 c_i(cc.LOSS_ID[loss]), c_d(c or 0.0), P(cov), P(s0), P(pc), P(st)) == 0
        cc.check_ragged(rc, mk, cov, s0, pc, fixed)
        cov2, s02 = np.full((B, 144), 5.0), np.full(B, 5.0)                    # without point_cov: the same cov and sigma0
        assert L.e_ba_cov_ragged(P(rc["packed"]), P(rc["off"]), c_l(B), c_l(nt), P(mk), P(rc["calms"]), c_l(27), P(rc["r2"]), P(rc["r3"]), P(rc["X"]), P(bounds),
                                 c_i(cc.LOSS_ID[loss]), c_d(c or 0.0), P(cov2), P(s02), None, P(st)) == 0
        assert cc.biteq(cov, cov2) and cc.biteq(s0, s02)
