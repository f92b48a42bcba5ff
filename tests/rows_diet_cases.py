"""
The scenes of tests/test_gpu_rows_diet.py and its GPU-less twin tests/test_emulated_rows_diet.py.

They sit where the trip structure of k_linear_tft_pose_rows (csrc/tft_rows_kernel.h) changes and tests/rows_lane_roles_cases.py (B = 7, N in {12, 200}
under its pin) does not look.  B = 5: a full wavefront and one live row.  N:
    16   the vote pass has only its first trip, the one that evaluates all four candidates; one moment trip (two half-bodies of eight
         correspondences each), both halves live on every lane pair;
    17   a second vote trip with one live lane; a second moment trip whose first half-body is live on one pair;
    24   the second moment trip's first half-body on every pair, its second half-body on none;
    25   ... its second half-body on one pair;
    33   a third moment trip, on one pair: a loop unrolled by two ends on its first member;
    40   ... on every pair, without a second half-body;
and one cell (KCELL_N correspondences) with a calibration matrix of its own for every view and every item (tests/rig_cases.py::per_view_K: skew,
K(3,3) != 1), so that the three calibration inverses and the first camera of rows_rt_prepare see three different general matrices.
A batch is the concatenation of scenes at sigma = 0, 1 and 3 px, as in rows_lane_roles_cases.scene; the per-view cell has 1 px throughout.

Seeds: 8300 + 1000 s + 10 B + N for the block of noise level number s; 8877 for the per-view cell.  tools/record_rows_diet.py refuses to write
the fixture unless every triplet has status 0.
"""
import functools

import numpy as np

B = 5
NS = (16, 17, 24, 25, 33, 40)
KCELL_N = 25
CELLS = tuple("n%d" % N for N in NS) + ("kview%d" % KCELL_N,)
SIGMAS = (0.0, 1.0, 3.0)
TOL = 1e-9                              # the gate of tests/test_gpu_parity.py
METHODS = ("LinearTFTPoseEstimation", "ResslTFTPoseEstimation")
PIN_KEYS = ("T", "R_t_2", "R_t_3", "Reconst", "status", "iter")


@functools.lru_cache(maxsize=None)
def scene(cell):
    """(Corresp (B, N, 6), CalM (9, 3), or (B, 9, 3) in the per-view cell).  Shared: do not write to it."""
    if cell.startswith("kview"):
        import rig_cases as RC
        C, CalM, _, _, _ = RC.rig_batch("converging", B, KCELL_N, 1.0, seed=8877, K="per_view")
    else:
        from tft_vs_fund_amd.scenes import generate_scene_batch
        N = int(cell[1:])
        blocks, CalM = [], None
        for s, sigma in enumerate(SIGMAS):
            nb = (B + 2 - s) // 3
            Cs, CalM, _, _ = generate_scene_batch(nb, N, noise=sigma, seed=8300 + 1000 * s + 10 * B + N)
            blocks.append(Cs)
        C = np.ascontiguousarray(np.concatenate(blocks, axis=0))
    assert C.shape[0] == B and C.shape[2] == 6
    C.setflags(write=False)
    CalM.setflags(write=False)
    return C, CalM


def calm_item(CalM, b):
    return CalM[b] if CalM.ndim == 3 else CalM


def calm_alone(CalM, b):
    """the calibration argument of a B = 1 call on item b"""
    return CalM[b:b + 1] if CalM.ndim == 3 else CalM


@functools.lru_cache(maxsize=None)
def oracle_linear(cell):
    """the oracle's (R_t_2, R_t_3, Reconst, T) of LinearTFTPoseEstimation for every triplet of scene(cell), computed once"""
    from oracle import tft_oracle as O
    C, CalM = scene(cell)
    return tuple(O.LinearTFTPoseEstimation(C[b].T.copy(), calm_item(CalM, b))[:4] for b in range(B))


def oracle_errors(method, cell, T, R_t_2, R_t_3, Reconst):
    """Worst relative deviation from the oracle per triplet: T (B,3,3,3) [b,j,k,i], R_t (B,3,4), Reconst (B,3,N).
    LinearTFT: the oracle's LinearTFTPoseEstimation, every output.
    Ressl: what the row kernels compute of it is the linear start and everything after the Gauss-Helmert iteration, and the oracle's own fp64
    evaluation of the iteration carries 1e-6 .. 1e-3 of noise (tests/test_gpu_gh_noise.py: pinv(W + 1e-12 I)), so a 1e-9 gate on T is a gate on
    the oracle.  Held at 1e-9 here: the poses against the oracle's R_t_from_TFT of the kernel's T with the item's calibration, and Reconst against
    the oracle's triangulation with those poses (the form tests/test_emulated_rigs.py uses); the bit pin of tests/test_gpu_rows_diet.py holds T."""
    from oracle import tft_oracle as O
    from helpers import rel_err_T, rel_err
    C, CalM = scene(cell)
    worst = []
    if method == "LinearTFTPoseEstimation":
        for b, (R2, R3, Rc, To) in enumerate(oracle_linear(cell)):
            worst.append(max(rel_err_T(T[b], To), rel_err(R_t_2[b], R2), rel_err(R_t_3[b], R3), rel_err(Reconst[b], Rc)))
        return worst
    for b in range(B):
        Cb, Kb = C[b].T.copy(), calm_item(CalM, b)
        R2, R3 = O.R_t_from_TFT(T[b], Kb, Cb)
        worst.append(max(rel_err(R_t_2[b], R2), rel_err(R_t_3[b], R3), rel_err(Reconst[b], O._final_reconst(Kb, R2, R3, Cb))))
    return worst


def gpu_outputs(ctx, method, C, CalM):
    """one pose_batch call on the device, outputs as numpy arrays"""
    import torch
    o = ctx.pose_batch(method, torch.from_numpy(np.array(C, order="C")).cuda(), torch.from_numpy(np.array(CalM, order="C")).cuda(), reconst=True)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in PIN_KEYS}


def record_pin(ctx):
    """the arrays of tests/golden/rows_diet_parent.npz from a context (tools/record_rows_diet.py)"""
    out = {}
    for method in METHODS:
        for cell in CELLS:
            C, CalM = scene(cell)
            for k, v in gpu_outputs(ctx, method, C, CalM).items():
                out["%s/%s/%s" % (method, cell, k)] = v
    return out
