"""
Lane roles of the four-triplet row kernels (csrc/tft_rows_kernel.h, f_rows_kernel.h) on the MI355X.  Their once-per-wavefront code decides what
a lane does from its position in its row of 16; the shapes (tests/rows_lane_roles_cases.py) are the ones at which that can go wrong:
B in {1, 5, 7} (live rows of the last wavefront: 1, 1 after a full one, 3) x N in {12, 27, 200}, every batch the concatenation of scenes at
sigma = 0, 1 and 3 px, so that the four rows of a wavefront leave the inverse iterations at different counts.

  * oracle: every triplet of LinearTFT and LinearF within 1e-9 of the oracle (the gate of tests/test_gpu_parity.py), every status 0;
  * travel invariance: a triplet's T, R_t_2, R_t_3, Reconst and status from the batch call equal, byte for byte, those of a B = 1 call on that
    triplet alone ("a triplet's result never depends on the wavefront it travels in");
  * bit pin: LinearTFT, LinearF and Ressl (its linear stage runs rows_linear_tft_middle) at B = 7, N in {12, 200} equal, byte for byte,
    tests/golden/rows_lane_roles_parent.npz -- the outputs of commit 421d831 (the parent of the lane-role work) on an MI355X, recorded with
        bash tools/build_ab_baseline.sh 421d831 P && python tools/record_rows_lane_roles.py tools/ab_libs/libtftfund_P.so
    A later change that moves bits ON PURPOSE records the fixture again from its own build (python tools/record_rows_lane_roles.py, no
    argument) and says so; one that is meant to keep results must leave this test alone.

tests/test_emulated_rows_lane_roles.py runs the first two checks on the lane emulator without a GPU.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rows_lane_roles_cases as cases   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_lane_roles_parent.npz")


@pytest.fixture(scope="module")
def gpu_ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    ctx = api.Context(0)
    ctx.set_rows(1)                                         # the row kernels at any batch size
    return ctx


@pytest.mark.parametrize("method", cases.METHODS)
@pytest.mark.parametrize("N", cases.NS)
@pytest.mark.parametrize("B", cases.BS)
def test_lane_roles_oracle_and_travel_invariance(gpu_ctx, method, B, N):
    C, CalM = cases.scene(B, N)
    o = cases.gpu_outputs(gpu_ctx, method, C, CalM)
    assert np.all(o["status"] == 0) and np.all(o["iter"] == 0), o["status"]
    errs = cases.oracle_errors(method, B, N, o["T"], o["R_t_2"], o["R_t_3"], o["Reconst"])
    print("%s B=%d N=%d worst deviation from the oracle %.3e" % (method, B, N, max(errs)))
    assert max(errs) < cases.TOL, errs
    if B > 1:
        for b in range(B):
            alone = cases.gpu_outputs(gpu_ctx, method, C[b:b + 1], CalM)
            for k in ("T", "R_t_2", "R_t_3", "Reconst", "status"):
                assert alone[k][0].tobytes() == o[k][b].tobytes(), (b, k)


@pytest.mark.parametrize("method", cases.PINNED)
@pytest.mark.parametrize("N", cases.PIN_NS)
def test_lane_roles_bit_pin(gpu_ctx, method, N):
    C, CalM = cases.scene(cases.PIN_B, N)
    o = cases.gpu_outputs(gpu_ctx, method, C, CalM)
    with np.load(GOLDEN) as pin:
        for k in cases.PIN_KEYS:
            want = pin["%s/n%d/%s" % (method, N, k)]
            assert o[k].dtype == want.dtype and o[k].shape == want.shape, k
            assert o[k].tobytes() == want.tobytes(), (k, int(np.sum(o[k] != want)))
