"""
The four-triplets-per-wavefront kernels of LinearTFT and LinearF (csrc/tft_rows_kernel.h, f_rows_kernel.h) at the correspondence counts where
their data passes change shape, on the MI355X:
    N = 12          only the masked tail group of the centroid pass (fewer than 64 correspondences), one 16-trip short of full
    N = 16, 17      exactly one full trip of 16, and one correspondence past it
    N = 24, 25      the second half-body (correspondences 8 .. 15 of a trip) of the moment loop's last trip present on every lane pair / on one
    N = 33          an odd number of trips: the ping-pong buffers of the moment loop end on the first pair
    N = 64, 65      whole 64-correspondence centroid groups only / one correspondence in the tail group
    N = 200         the benchmark's own trip counts
B = 9: three wavefronts, the last with one live row.  Sigma = 1 px.  Every triplet against the oracle (1e-9, the gate of tests/test_gpu_parity.py)
and against the one-triplet-per-wavefront route (TFF_OPT_ROWS = 0) at the tolerances of tests/test_gpu_rows.py; every status 0.
tests/test_emulated_rows_boundaries.py runs the same scenes through the emulated kernels without a GPU.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import rel_err_T, rel_err   # noqa: E402

TOL = 1e-9
B = 9
NS = [12, 13, 16, 17, 24, 25, 33, 64, 65, 200]


def boundary_scene(N):
    """the seeded scene of one N, shared with the emulated twin"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(B, N, noise=1.0, seed=4100 + N)
    return C, CalM


@pytest.fixture(scope="module")
def gpu_ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    ctx = api.Context(0)
    ctx.set_rows(1)
    return ctx


@pytest.mark.parametrize("method", ["LinearTFTPoseEstimation", "LinearFPoseEstimation"])
@pytest.mark.parametrize("N", NS)
def test_rows_route_at_trip_boundaries(gpu_ctx, method, N):
    import torch
    from oracle import tft_oracle as O
    C, CalM = boundary_scene(N)
    d = torch.from_numpy(C).cuda(); calm = torch.from_numpy(CalM).cuda()
    out = {}
    for rows in (1, 0):
        gpu_ctx.set_rows(rows)
        try:
            o = gpu_ctx.pose_batch(method, d, calm, reconst=True)
        finally:
            gpu_ctx.set_rows(1)
        out[rows] = {k: v.cpu().numpy() for k, v in o.items() if k != "_raw" and v is not None and hasattr(v, "cpu")}
    r, w = out[1], out[0]
    assert np.all(r["status"] == 0) and np.all(w["status"] == 0) and np.all(r["iter"] == 0)
    for b in range(B):
        R2, R3, Rec, T, _ = getattr(O, method)(C[b].T.copy(), CalM)
        errs = (rel_err_T(r["T"][b], T), rel_err(r["R_t_2"][b], R2), rel_err(r["R_t_3"][b], R3), rel_err(r["Reconst"][b], Rec))
        assert max(errs) < TOL, (b, errs)
    sg = np.sign(np.sum(r["T"] * w["T"], axis=(1, 2, 3)))[:, None, None, None]
    assert np.abs(r["T"] * sg - w["T"]).max() < TOL
    assert np.abs(r["R_t_2"] - w["R_t_2"]).max() < TOL
    assert np.abs(r["R_t_3"] - w["R_t_3"]).max() < TOL * max(1.0, np.abs(w["R_t_3"]).max())
    assert np.abs(r["Reconst"] - w["Reconst"]).max() < 1e-8 * np.abs(w["Reconst"]).max()
