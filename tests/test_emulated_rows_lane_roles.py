"""
The GPU-less twin of tests/test_gpu_rows_lane_roles.py: the same seeded scenes (tests/rows_lane_roles_cases.py: B in {1, 5, 7} x N in {12, 27, 200},
sigma = 0 / 1 / 3 px in one batch) through the emulated k_linear_tft_pose_rows / k_linear_f_pose_rows (tests/emu):
  * every triplet against the oracle at 1e-9 and every status 0;
  * travel invariance: a triplet's T, R_t_2, R_t_3, Reconst and status from the batch call equal, byte for byte, those of a B = 1 call on that
    triplet alone ("a triplet's result never depends on the wavefront it travels in").
"""
import ctypes

import numpy as np
import pytest

from tft_vs_fund_amd.scenes import calm_colmajor
from emu import emu_build
import rows_lane_roles_cases as cases

ENTRY = {"LinearTFTPoseEstimation": "emu_linear_tft_pose_rows", "LinearFPoseEstimation": "emu_linear_f_pose_rows"}


@pytest.fixture(scope="module")
def emu():
    return emu_build.load()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _run(emu, method, C, CalM):
    C = np.ascontiguousarray(C)
    B, N = C.shape[0], C.shape[1]
    calm = calm_colmajor(CalM)
    o = dict(Rt2=np.zeros((B, 12)), Rt3=np.zeros((B, 12)), T=np.zeros((B, 27)), Rec=np.zeros((B, N, 3)), it=np.zeros(B, dtype=np.int32),
             st=np.ones(B, dtype=np.int32))
    getattr(emu, ENTRY[method])(_p(C), _p(calm), ctypes.c_long(0), ctypes.c_long(B), ctypes.c_int(N), ctypes.c_int(0), _p(o["Rt2"]), _p(o["Rt3"]),
                                _p(o["T"]), _p(o["Rec"]), _p(o["it"]), _p(o["st"]), None)
    return o


@pytest.mark.parametrize("method", cases.METHODS)
@pytest.mark.parametrize("N", cases.NS)
@pytest.mark.parametrize("B", cases.BS)
def test_emulated_lane_roles(emu, method, B, N):
    C, CalM = cases.scene(B, N)
    o = _run(emu, method, C, CalM)
    assert np.all(o["st"] == 0) and np.all(o["it"] == 0), o["st"]
    errs = cases.oracle_errors(method, B, N, o["T"].reshape(B, 3, 3, 3).transpose(0, 3, 2, 1), o["Rt2"].reshape(B, 4, 3).transpose(0, 2, 1),
                               o["Rt3"].reshape(B, 4, 3).transpose(0, 2, 1), o["Rec"].transpose(0, 2, 1))
    print("%s B=%d N=%d worst deviation from the oracle %.3e" % (method, B, N, max(errs)))
    assert max(errs) < cases.TOL, errs
    if B > 1:
        for b in range(B):
            alone = _run(emu, method, C[b:b + 1], CalM)
            for k in ("T", "Rt2", "Rt3", "Rec", "st"):
                assert alone[k][0].tobytes() == o[k][b].tobytes(), (b, k)
