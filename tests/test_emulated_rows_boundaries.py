"""
The GPU-less twin of tests/test_gpu_rows_boundaries.py: the same seeded scenes (B = 9, sigma = 1 px, the correspondence counts at which the data
passes of the row kernels change shape) through the emulated k_linear_tft_pose_rows / k_linear_f_pose_rows (tests/emu), every triplet against
the oracle at 1e-9 and every status 0.
"""
import ctypes

import numpy as np
import pytest

from oracle import tft_oracle as O
from tft_vs_fund_amd.scenes import calm_colmajor
from helpers import rel_err_T, rel_err
from emu import emu_build
from test_gpu_rows_boundaries import B, NS, boundary_scene


@pytest.fixture(scope="module")
def emu():
    return emu_build.load()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("method,entry", [("LinearTFTPoseEstimation", "emu_linear_tft_pose_rows"), ("LinearFPoseEstimation", "emu_linear_f_pose_rows")])
@pytest.mark.parametrize("N", NS)
def test_emulated_rows_kernels_at_trip_boundaries(emu, method, entry, N):
    C, CalM = boundary_scene(N)
    calm = calm_colmajor(CalM)
    Rt2 = np.zeros((B, 12)); Rt3 = np.zeros((B, 12)); T = np.zeros((B, 27)); Rec = np.zeros((B, N, 3))
    it = np.zeros(B, dtype=np.int32); st = np.ones(B, dtype=np.int32)
    getattr(emu, entry)(_p(C), _p(calm), ctypes.c_long(0), ctypes.c_long(B), ctypes.c_int(N), ctypes.c_int(0), _p(Rt2), _p(Rt3), _p(T), _p(Rec),
                        _p(it), _p(st), None)
    assert np.all(st == 0) and np.all(it == 0)
    R_t_2 = Rt2.reshape(B, 4, 3).transpose(0, 2, 1); R_t_3 = Rt3.reshape(B, 4, 3).transpose(0, 2, 1)
    Tt = T.reshape(B, 3, 3, 3).transpose(0, 3, 2, 1); Reconst = Rec.transpose(0, 2, 1)
    for b in range(B):
        R2, R3, Rc, To, _ = getattr(O, method)(C[b].T.copy(), CalM)
        errs = (rel_err_T(Tt[b], To), rel_err(R_t_2[b], R2), rel_err(R_t_3[b], R3), rel_err(Reconst[b], Rc))
        assert max(errs) < 1e-9, (b, errs)
