"""
The GPU-less twin of tests/test_gpu_rows_diet.py: the same seeded scenes (tests/rows_diet_cases.py: B = 5, N in {16, 17, 24, 25, 33, 40}, sigma = 0 / 1 / 3 px
in one batch, and one cell with a general calibration matrix per view and item) through the emulated k_linear_tft_pose_rows and the emulated
Gauss-Helmert chain of Ressl, whose linear stage and pose tail are the row kernels' (tests/emu):
  * every triplet against the oracle at 1e-9 (rows_diet_cases.oracle_errors) and every status 0;
  * travel invariance: a triplet's T, R_t_2, R_t_3, Reconst, iter and status from the batch call equal, byte for byte, those of a B = 1 call on that
    triplet alone ("a triplet's result never depends on the wavefront it travels in").
"""
import ctypes

import numpy as np
import pytest

from emu import emu_build
import rows_diet_cases as cases


@pytest.fixture(scope="module")
def emu():
    return emu_build.load()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _run(emu, method, C, CalM):
    C = np.ascontiguousarray(C)
    B, N = C.shape[0], C.shape[1]
    CalM = np.asarray(CalM, dtype=np.float64)
    if CalM.ndim == 2:                                       # column-major doubles and the stride between items, as the C ABI takes them
        calm, stride = np.ascontiguousarray(CalM.T).reshape(-1), 0
    else:
        calm, stride = np.ascontiguousarray(CalM.transpose(0, 2, 1)).reshape(-1), CalM.shape[1] * 3
    o = dict(Rt2=np.zeros((B, 12)), Rt3=np.zeros((B, 12)), T=np.zeros((B, 27)), Rec=np.zeros((B, N, 3)), it=np.zeros(B, dtype=np.int32),
             st=np.ones(B, dtype=np.int32))
    head = (_p(C), _p(calm), ctypes.c_long(stride), ctypes.c_long(B), ctypes.c_int(N), ctypes.c_int(0))
    outs = (_p(o["Rt2"]), _p(o["Rt3"]), _p(o["T"]), _p(o["Rec"]), _p(o["it"]), _p(o["st"]))
    if method == "ResslTFTPoseEstimation":
        emu.emu_gh_wg_pose(ctypes.c_int(0), *head, *outs)
    else:
        emu.emu_linear_tft_pose_rows(*head, *outs, None)
    return o


@pytest.mark.parametrize("method", cases.METHODS)
@pytest.mark.parametrize("cell", cases.CELLS)
def test_emulated_rows_diet(emu, method, cell):
    C, CalM = cases.scene(cell)
    B = cases.B
    o = _run(emu, method, C, CalM)
    assert np.all(o["st"] == 0), o["st"]
    errs = cases.oracle_errors(method, cell, o["T"].reshape(B, 3, 3, 3).transpose(0, 3, 2, 1), o["Rt2"].reshape(B, 4, 3).transpose(0, 2, 1),
                               o["Rt3"].reshape(B, 4, 3).transpose(0, 2, 1), o["Rec"].transpose(0, 2, 1))
    print("%s %s worst deviation from the oracle %.3e" % (method, cell, max(errs)))
    assert max(errs) < cases.TOL, errs
    for b in range(B):
        alone = _run(emu, method, C[b:b + 1], cases.calm_alone(CalM, b))
        for k in ("T", "Rt2", "Rt3", "Rec", "it", "st"):
            assert alone[k][0].tobytes() == o[k][b].tobytes(), (b, k)
