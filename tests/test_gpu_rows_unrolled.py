"""
The four-triplets-per-wavefront kernels of LinearTFT and LinearF (csrc/tft_rows_kernel.h, f_rows_kernel.h) at the correspondence counts and batch
sizes that tests/test_gpu_rows_boundaries.py does not hold, on the MI355X:
    N = 7, 8, 9     the minimal sizes (exact tiers; the moment loop of the fast tier would run a first half-body only)
    N = 32, 40      an even number of moment trips (two), without and with the second half-body of the last one
    N = 41, 48, 49  three and four moment trips: a pair of trips ends on its first / on its second member
    B = 1, 4, 5, 9  one live row, a full wavefront, a wavefront with a single live row behind a full one (once and twice)
Sigma = 1 px, Reconst on.  Every triplet against the oracle -- 1e-9 (the gate of tests/test_gpu_parity.py) and status 0 for N >= 12; below 12 the
minimal-sample gate of that file (1e-6) under the best of the 16 svd(E) sign conventions (tests/helpers.py::pose_err_any_convention's references) --
and against the one-triplet-per-wavefront route (TFF_OPT_ROWS = 0) at the tolerances of tests/test_gpu_rows.py (1e-9, Reconst 1e-8; minimal samples
1e-7 on T and 1e-6 on R_t_3 as in test_exact_rows_kernel_against_the_one_triplet_exact_kernel).  One ragged call mixes all these N and is compared
bit for bit with the fixed-N calls, as tests/test_gpu_ragged.py does.
tests/test_emulated_rows_unrolled.py runs the same scenes through the emulated kernels without a GPU.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import rel_err, pose_err, oracle_under_conventions   # noqa: E402

TOL = 1e-9
TOL_MINIMAL = 1e-6
NS = [7, 8, 9, 32, 40, 41, 48, 49]
BS = [1, 4, 5, 9]
BMAX = max(BS)
METHODS = ["LinearTFTPoseEstimation", "LinearFPoseEstimation"]


@functools.lru_cache(maxsize=None)
def unrolled_scene(N):
    """the seeded scene of one N (BMAX triplets; a batch of B takes the first B), shared with the emulated twin"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(BMAX, N, noise=1.0, seed=5200 + N)
    return C, CalM


@functools.lru_cache(maxsize=None)
def oracle_refs(method, N, b):
    """the oracle's result(s) for triplet b of unrolled_scene(N): one for N >= 12, the 16 svd(E) sign conventions for a minimal sample"""
    from oracle import tft_oracle as O
    C, CalM = unrolled_scene(N)
    fn = getattr(O, method)
    if N >= 12:
        return [fn(C[b].T.copy(), CalM)]
    return [r for r in oracle_under_conventions(fn, C[b].T.copy(), CalM) if r is not None]


def check_against_oracle(method, N, B, out):
    """out: dict of numpy arrays (T, R_t_2, R_t_3, Reconst (B,3,N), status) for the first B triplets of unrolled_scene(N)"""
    if method == "LinearFPoseEstimation" and N < 8:                          # linearF.m:35-37
        assert np.all(out["status"] == 1) and np.isnan(out["T"]).all()
        return
    assert np.all(out["status"] == 0), out["status"]
    for b in range(B):
        ob = {k: out[k][b] for k in ("T", "R_t_2", "R_t_3")}
        refs = oracle_refs(method, N, b)
        errs = [max(pose_err(ob, r), rel_err(out["Reconst"][b], r[2])) for r in refs]
        assert min(errs) < (TOL if N >= 12 else TOL_MINIMAL), (N, B, b, errs[0], min(errs))


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items() if k != "_raw" and v is not None and hasattr(v, "cpu")}


@pytest.fixture(scope="module")
def gpu_ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    ctx = api.Context(0)
    ctx.set_rows(1)
    return ctx


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("N", NS)
def test_rows_route_at_unrolled_loop_shapes(gpu_ctx, method, N, B):
    import torch
    C, CalM = unrolled_scene(N)
    d = torch.from_numpy(np.ascontiguousarray(C[:B])).cuda(); calm = torch.from_numpy(CalM).cuda()
    out = {}
    for rows in (1, 0):
        gpu_ctx.set_rows(rows)
        try:
            out[rows] = _np(gpu_ctx.pose_batch(method, d, calm, reconst=True))
        finally:
            gpu_ctx.set_rows(1)
    r, w = out[1], out[0]
    assert np.array_equal(r["status"], w["status"]) and np.all(r["iter"] == 0)
    check_against_oracle(method, N, B, r)
    if np.all(r["status"] != 0):
        return
    sg = np.sign(np.sum(r["T"] * w["T"], axis=(1, 2, 3)))[:, None, None, None]
    eT = np.abs(r["T"] * sg - w["T"]).max()
    e2 = np.abs(r["R_t_2"] - w["R_t_2"]).max()
    e3 = np.abs(r["R_t_3"] - w["R_t_3"]).max() / max(1.0, np.abs(w["R_t_3"]).max())
    eX = np.abs(r["Reconst"] - w["Reconst"]).max() / np.abs(w["Reconst"]).max()
    print("N=%d B=%d %s: rows vs one-triplet route T %.2e R_t_2 %.2e R_t_3 %.2e Reconst %.2e" % (N, B, method, eT, e2, e3, eX))
    if N >= 12:
        assert eT < TOL and e2 < TOL and e3 < TOL and eX < 1e-8
    else:
        assert eT < 1e-7 and e3 < 1e-6


@pytest.mark.parametrize("method", METHODS)
def test_ragged_call_mixing_these_sizes_equals_the_fixed_n_calls_bit_for_bit(gpu_ctx, method):
    import torch
    from tft_vs_fund_amd import api
    items, ref = [], []
    CalM = unrolled_scene(NS[0])[1]
    for N in NS:
        C, cm = unrolled_scene(N)
        assert np.array_equal(cm, CalM)
        o = _np(gpu_ctx.pose_batch(method, torch.from_numpy(C).cuda(), torch.from_numpy(CalM).cuda(), reconst=True))
        for b in range(BMAX):
            items.append(np.ascontiguousarray(C[b]))
            ref.append({k: o[k][b] for k in ("T", "R_t_2", "R_t_3", "Reconst", "iter", "status")})
    perm = np.random.default_rng(3).permutation(len(items))
    items = [items[i] for i in perm]; ref = [ref[i] for i in perm]
    corresp, offsets = api.pack_ragged(items)
    o = _np(gpu_ctx.pose_batch_ragged(method, torch.from_numpy(corresp).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(CalM).cuda(), reconst=True))
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    for b in range(len(items)):
        for k in ("T", "R_t_2", "R_t_3"):
            assert np.array_equal(bits(o[k][b]), bits(ref[b][k])), (b, len(items[b]), k)
        assert np.array_equal(bits(o["Reconst"][offsets[b]:offsets[b + 1]]), bits(ref[b]["Reconst"].T)), (b, len(items[b]))
        assert o["iter"][b] == ref[b]["iter"] and o["status"][b] == ref[b]["status"], (b, len(items[b]))
