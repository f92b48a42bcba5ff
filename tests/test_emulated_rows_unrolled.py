"""
The GPU-less twin of tests/test_gpu_rows_unrolled.py: the same seeded scenes (sigma = 1 px; N = 7, 8, 9, 32, 40, 41, 48, 49; B = 1, 4, 5, 9) through
the emulated row kernels (tests/emu) as the library routes them -- k_linear_tft_pose_rows / k_linear_f_pose_rows for N >= 12, their exact tiers
below -- every triplet against the oracle at the gates of the GPU twin (1e-9 and status 0 for N >= 12, the minimal-sample gate below).
Every N runs at B = 5 (a full wavefront and one with a single live row), every B at N = 41 and at N = 8.
"""
import ctypes

import numpy as np
import pytest

from tft_vs_fund_amd.scenes import calm_colmajor
from emu import emu_build
from test_gpu_rows_unrolled import NS, BS, unrolled_scene, check_against_oracle

ENTRIES = {("LinearTFTPoseEstimation", False): "emu_linear_tft_pose_rows", ("LinearTFTPoseEstimation", True): "emu_linear_tft_pose_rows_exact",
           ("LinearFPoseEstimation", False): "emu_linear_f_pose_rows", ("LinearFPoseEstimation", True): "emu_linear_f_pose_rows_exact"}
CASES = sorted(set([(N, 5) for N in NS] + [(41, B) for B in BS] + [(8, B) for B in BS]))


@pytest.fixture(scope="module")
def emu():
    return emu_build.load()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("method", ["LinearTFTPoseEstimation", "LinearFPoseEstimation"])
@pytest.mark.parametrize("N,B", CASES)
def test_emulated_rows_kernels_at_unrolled_loop_shapes(emu, method, N, B):
    C, CalM = unrolled_scene(N)
    C = np.ascontiguousarray(C[:B])
    calm = calm_colmajor(CalM)
    Rt2 = np.zeros((B, 12)); Rt3 = np.zeros((B, 12)); T = np.zeros((B, 27)); Rec = np.zeros((B, N, 3))
    it = np.zeros(B, dtype=np.int32); st = np.full(B, -1, dtype=np.int32)
    getattr(emu, ENTRIES[(method, N < 12)])(_p(C), _p(calm), ctypes.c_long(0), ctypes.c_long(B), ctypes.c_int(N), ctypes.c_int(0), _p(Rt2), _p(Rt3), _p(T),
                                            _p(Rec), _p(it), _p(st), None)
    assert np.all(it == 0)
    out = {"R_t_2": Rt2.reshape(B, 4, 3).transpose(0, 2, 1), "R_t_3": Rt3.reshape(B, 4, 3).transpose(0, 2, 1),
           "T": T.reshape(B, 3, 3, 3).transpose(0, 3, 2, 1), "Reconst": Rec.transpose(0, 2, 1), "status": st}
    check_against_oracle(method, N, B, out)
