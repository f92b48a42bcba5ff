"""
The trip structure of k_linear_tft_pose_rows (csrc/tft_rows_kernel.h) on the MI355X, at the sizes where it changes (tests/rows_diet_cases.py: B = 5,
N in {16, 17, 24, 25, 33, 40}, sigma = 0 / 1 / 3 px in one batch, and one cell with a general calibration matrix per view and item):

  * oracle: every triplet of LinearTFT, and of Ressl what the row kernels compute of it, within 1e-9 of the oracle (rows_diet_cases.oracle_errors),
    every status 0;
  * bit pin: LinearTFT and Ressl equal, byte for byte, tests/golden/rows_diet_parent.npz -- the outputs of commit b2643a9 (the parent of the change
    that unrolled the moment loop) on an MI355X, recorded with
        bash tools/build_ab_baseline.sh b2643a9 P && python tools/record_rows_diet.py tools/ab_libs/libtftfund_P.so
    A change that is meant to keep results must leave this test and its fixture alone.

tests/test_emulated_rows_diet.py runs the oracle check and travel invariance on the lane emulator without a GPU.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rows_diet_cases as cases   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_diet_parent.npz")


@pytest.fixture(scope="module")
def gpu_ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    ctx = api.Context(0)
    ctx.set_rows(1)                                         # the row kernels at any batch size
    return ctx


@pytest.mark.parametrize("method", cases.METHODS)
@pytest.mark.parametrize("cell", cases.CELLS)
def test_rows_diet_oracle_and_bit_pin(gpu_ctx, method, cell):
    C, CalM = cases.scene(cell)
    o = cases.gpu_outputs(gpu_ctx, method, C, CalM)
    assert np.all(o["status"] == 0), o["status"]
    errs = cases.oracle_errors(method, cell, o["T"], o["R_t_2"], o["R_t_3"], o["Reconst"])
    print("%s %s worst deviation from the oracle %.3e" % (method, cell, max(errs)))
    assert max(errs) < cases.TOL, errs
    with np.load(GOLDEN) as pin:
        for k in cases.PIN_KEYS:
            want = pin["%s/%s/%s" % (method, cell, k)]
            if k == "status":
                assert np.all(want == 0), want                                # the scenes have status 0 on the parent
            assert o[k].dtype == want.dtype and o[k].shape == want.shape, k
            assert o[k].tobytes() == want.tobytes(), (k, int(np.sum(o[k] != want)))
