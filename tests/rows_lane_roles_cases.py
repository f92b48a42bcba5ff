"""
The scenes of tests/test_gpu_rows_lane_roles.py and its GPU-less twin tests/test_emulated_rows_lane_roles.py.

What the once-per-wavefront code of the four-triplet row kernels depends on is not the trip count but the lane roles: the 16 positions of a row,
the p < 11 split of the 27 x 27 solve, how many rows of the last wavefront own a triplet, and four rows that iterate different numbers of times
in one instruction stream.  So: B in {1, 5, 7} (one live row; a full wavefront and one live row; a full wavefront and three) x N in {12, 27, 200}
(only the masked tail group of the centroid pass; 27 = the order of the first solve; the benchmark's count), and a batch is the concatenation of
three generate_scene_batch calls at sigma = 0, 1 and 3 px, so that neighbouring rows need different inverse-iteration counts.

Seeds: 7300 + 1000 s + 10 B + N for the block of noise level number s (0, 1, 2).  With these every triplet has status 0 at the commit before the
lane-role work (421d831), in LinearTFT and in LinearF, on the lane emulator and on the MI355X.
"""
import functools

import numpy as np

BS = (1, 5, 7)
NS = (12, 27, 200)
SIGMAS = (0.0, 1.0, 3.0)
TOL = 1e-9                              # the gate of tests/test_gpu_parity.py
METHODS = ("LinearTFTPoseEstimation", "LinearFPoseEstimation")
PINNED = ("LinearTFTPoseEstimation", "LinearFPoseEstimation", "ResslTFTPoseEstimation")
PIN_B, PIN_NS = 7, (12, 200)
PIN_KEYS = ("T", "R_t_2", "R_t_3", "Reconst", "status", "iter")


@functools.lru_cache(maxsize=None)
def scene(B, N):
    """(Corresp (B, N, 6), CalM): blocks of (B + 2) // 3, (B + 1) // 3 and B // 3 triplets at sigma = 0, 1 and 3 px.  Shared: do not write to it."""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    blocks, CalM = [], None
    for s, sigma in enumerate(SIGMAS):
        nb = (B + 2 - s) // 3
        if nb == 0:
            continue
        C, CalM, _, _ = generate_scene_batch(nb, N, noise=sigma, seed=7300 + 1000 * s + 10 * B + N)
        blocks.append(C)
    C = np.ascontiguousarray(np.concatenate(blocks, axis=0))
    assert C.shape == (B, N, 6)
    C.setflags(write=False)
    return C, CalM


@functools.lru_cache(maxsize=None)
def oracle(method, B, N):
    """the oracle's (R_t_2, R_t_3, Reconst, T) of every triplet of scene(B, N), computed once"""
    from oracle import tft_oracle as O
    C, CalM = scene(B, N)
    return tuple(getattr(O, method)(C[b].T.copy(), CalM)[:4] for b in range(B))


def oracle_errors(method, B, N, T, R_t_2, R_t_3, Reconst):
    """worst relative deviation from the oracle per triplet: T (B,3,3,3) [b,j,k,i], R_t (B,3,4), Reconst (B,3,N)"""
    from helpers import rel_err_T, rel_err
    worst = []
    for b, (R2, R3, Rc, To) in enumerate(oracle(method, B, N)):
        worst.append(max(rel_err_T(T[b], To), rel_err(R_t_2[b], R2), rel_err(R_t_3[b], R3), rel_err(Reconst[b], Rc)))
    return worst


def gpu_outputs(ctx, method, C, CalM):
    """one pose_batch call on the device, outputs as numpy arrays"""
    import torch
    o = ctx.pose_batch(method, torch.from_numpy(np.array(C, order="C")).cuda(), torch.from_numpy(CalM).cuda(), reconst=True)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in PIN_KEYS}


def record_pin(ctx):
    """the arrays of tests/golden/rows_lane_roles_parent.npz from a context (tools/record_rows_lane_roles.py)"""
    out = {}
    for method in PINNED:
        for N in PIN_NS:
            C, CalM = scene(PIN_B, N)
            for k, v in gpu_outputs(ctx, method, C, CalM).items():
                out["%s/n%d/%s" % (method, N, k)] = v
    return out
