"""
The bundle adjustment over tracks with a robust loss (csrc/ba_tracks_loss_kernel.h: k_bundle_adjust_tracks_loss<2 .. 6, Huber | Cauchy>) on the lane
emulator, no GPU, compiled by g++ (tests/emu/emu_ba_tracks_loss.cpp), against the numpy restatement (tests/ba_tracks_loss_oracle.py) over the cases of
tests/ba_tracks_loss_cases.py at its gate: status and used exact, iter equal, repr_err, R_t and the Reconst columns of the points taking part within
1e-9 relative, the weights within 1e-9 absolute, NaN exactly where rule 7 of include/tftfund_tracks_loss.h says.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ba_tracks_cases as tc
import ba_tracks_loss_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i, c_d = ctypes.c_long, ctypes.c_int, ctypes.c_double
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
LOSS_ID = {None: 0, "huber": 1, "cauchy": 2}


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_ba_tracks_loss.so")
    deps = [os.path.join(emu, f) for f in ("emu_ba_tracks_loss.cpp", "emu_primitives.h", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_ba_tracks_loss.cpp")], check=True)
    return ctypes.CDLL(out)


def run(L, CalM, R0, C, X0, loss, scale, outputs=True):
    """the emulated call, B = 1 -> dict as ba_tracks_loss_cases.gate takes it"""
    M, N = C.shape[0] // 2, C.shape[1]
    calm = np.ascontiguousarray(CalM.T).reshape(-1); rt = np.ascontiguousarray(R0.T).reshape(-1); Cc = np.ascontiguousarray(C.T)
    x0 = np.ascontiguousarray(X0.T) if X0 is not None else None
    out = np.full(12 * M, 5.0); rec = np.full((N, 3), 5.0); it = np.full(1, 5, dtype=np.int32); err = np.full(1, 5.0)
    used = np.full(1, -5, dtype=np.int32); st = np.full(1, 5, dtype=np.int32); w = np.full((N, M), 5.0)
    sc = c_d(0.0 if scale is None else scale)
    if outputs:
        assert L.e_ba_tracks_loss(M, P(calm), c_l(0), P(rt), P(Cc), c_l(1), c_i(N), P(x0), P(out), P(rec), P(it), P(err), P(used), P(st), LOSS_ID[loss], sc, P(w)) == 0
    else:                                                                                # every output but Rt may be NULL
        assert L.e_ba_tracks_loss(M, P(calm), c_l(0), P(rt), P(Cc), c_l(1), c_i(N), P(x0), P(out), None, None, None, None, None, LOSS_ID[loss], sc, None) == 0
    return dict(R_t=out.reshape(4, 3 * M).T, Reconst=rec.T, iter=int(it[0]), repr_err=float(err[0]), used=int(used[0]), status=int(st[0]), weight=w)


def same_bits(a, b, n=None):
    """two runs agree in every bit (b possibly padded beyond n columns)"""
    n = a["Reconst"].shape[1] if n is None else n
    return (a["iter"], a["used"], a["status"]) == (b["iter"], b["used"], b["status"]) and np.array([a["repr_err"]]).tobytes() == np.array([b["repr_err"]]).tobytes() \
        and a["R_t"].tobytes() == b["R_t"].tobytes() and np.ascontiguousarray(a["Reconst"][:, :n]).tobytes() == np.ascontiguousarray(b["Reconst"][:, :n]).tobytes() \
        and np.ascontiguousarray(a["weight"][:n]).tobytes() == np.ascontiguousarray(b["weight"][:n]).tobytes()


@pytest.mark.parametrize("M,N,pattern,loss,c", lc.COMPARED)
def test_kernel_matches_the_restatement(M, N, pattern, loss, c):
    ref = lc.restated(M, N, pattern, loss, c)
    assert lc.compared(ref), (ref["iter"], ref["margins"])
    CalM, R0, C, X0, _ = lc.inputs(M, N, pattern)
    lc.gate(run(_lib(), CalM, R0, C, X0, loss, c), ref, (M, N, pattern, loss, c))


@pytest.mark.parametrize("loss,c", lc.LOSSES)
def test_the_fifth_instance_pair(loss, c):
    """M = 5 is not on the grid of ba_tracks_cases: one partially visible case for each of its two instances"""
    CalM, R0, C, X0 = tc.scene(5, 65)
    C = tc.apply_pattern(C, "random"); C[2:4, 7] += 45.0
    ref = lc.TLO.ba_tracks_loss(CalM, R0, C, None, loss, c)
    assert lc.compared(ref)
    lc.gate(run(_lib(), CalM, R0, C, None, loss, c), ref, (5, loss))


@pytest.mark.parametrize("kind", tc.FAILING)
@pytest.mark.parametrize("loss,c", lc.LOSSES + ((None, None),))
def test_failing_items(kind, loss, c):
    case, used, status = tc.failing(kind)
    got = run(_lib(), *case, loss, c)
    assert (got["used"], got["status"]) == (used, status)
    lc.gate(got, lc.restated_failing(kind, loss, c), (kind, loss))


def test_loss_none_is_the_plain_kernel_and_its_weights_are_one_or_nan():
    import test_emulated_ba_tracks as plain
    L = _lib()
    for M, N, pattern in ((3, 65, "random"), (6, 130, "few_obs")):
        CalM, R0, C, X0, _ = lc.inputs(M, N, pattern)
        a = run(L, CalM, R0, C, X0, None, None)
        R_t, X, it, err, used, st = plain.run(plain._lib(), CalM, R0, C, X0)
        assert (a["iter"], a["used"], a["status"]) == (it, used, st) and a["repr_err"] == err
        assert a["R_t"].tobytes() == R_t.tobytes() and np.ascontiguousarray(a["Reconst"]).tobytes() == np.ascontiguousarray(X).tobytes()
        vis = lc.TO.visibility(C)
        want = np.where(vis & (vis.sum(axis=0) >= 2)[None], 1.0, np.nan).T
        assert np.array_equal(a["weight"], want, equal_nan=True) and np.isnan(want).any() and (want == 1.0).any()


def test_an_unseen_view_keeps_its_pose_and_null_outputs_change_nothing():
    L = _lib()
    M, N = 4, 65
    CalM, R0, C, X0, _ = lc.inputs(M, N, "view_nan")
    a = run(L, CalM, R0, C, X0, "cauchy", 3.0)
    assert a["status"] == 0 and a["used"] == N and np.isnan(a["weight"][:, M - 1]).all() and np.isfinite(a["weight"][:, :M - 1]).all()
    R_t = a["R_t"]
    G = np.vstack([R0[0:3], [0, 0, 0, 1]])                                               # the frame of camera 1 (BundleAdjustment.m:80-86)
    start = R0[3 * (M - 1):3 * M] @ np.linalg.inv(G)
    sc = np.linalg.norm(R_t[3 * (M - 1):3 * M, 3]) / np.linalg.norm(start[:, 3])
    assert np.abs(R_t[3 * (M - 1):3 * M, :3] - start[:, :3]).max() < 1e-12 and np.abs(R_t[3 * (M - 1):3 * M, 3] - sc * start[:, 3]).max() < 1e-12
    assert abs(np.linalg.norm(R_t[3:6, 3]) - 1) < 1e-12
    assert run(L, CalM, R0, C, X0, "cauchy", 3.0, outputs=False)["R_t"].tobytes() == R_t.tobytes()
    assert L.e_ba_tracks_loss(7, *([None] * 3), None, c_l(1), c_i(N), *([None] * 7), 1, c_d(1.0), None) == -1     # no seventh view, no fourth loss
    assert L.e_ba_tracks_loss(3, *([None] * 3), None, c_l(1), c_i(N), *([None] * 7), 3, c_d(1.0), None) == -1


@pytest.mark.parametrize("M,N1", [(3, 130), (6, 130)])
def test_appended_nan_columns_change_no_bit(M, N1):
    """the padding that serves as the ragged form of this call: N = 65 padded to 130 equals N = 65, weights included"""
    L = _lib()
    N0 = 65
    CalM, R0, C, X0, _ = lc.inputs(M, N0, "random")
    assert X0 is None
    for loss, c in lc.LOSSES:
        a = run(L, CalM, R0, C, None, loss, c)
        b = run(L, CalM, R0, np.hstack([C, np.full((2 * M, N1 - N0), np.nan)]), None, loss, c)
        assert same_bits(a, b, N0) and np.isnan(b["Reconst"][:, N0:]).all() and np.isnan(b["weight"][N0:]).all()
