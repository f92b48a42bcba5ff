"""
TEST INFRASTRUCTURE ONLY -- the scenes of the robust-loss bundle adjustment tests (tests/test_ba_loss_cpu.py, tests/test_emulated_ba_loss.py,
tests/test_gpu_ba_loss.py) and their restated results (tests/ba_loss_oracle.py), computed once per process.

A scene: generate_scene_batch with 1 px of noise; `n_bad` of its matches displaced by 20 .. 80 px, either sign, in all six coordinates; the start is
the ground truth (scale |t2| = 1) turned by 0.02 rad about a random axis per camera, its translations off by 2 %; start points within 1 % of the truth.
"""
import functools

import numpy as np

import ba_loss_oracle as LO
from tft_vs_fund_amd.scenes import generate_scene_batch, scene_cameras

# (matches, displaced): trips of one, one, one, two and a bit wavefronts
SIZES = ((12, 0), (40, 2), (64, 8), (65, 13), (129, 0))
LOSSES = (("huber", 3.0), ("huber", 1.5), ("cauchy", 3.0), ("cauchy", 1.5))
CASES = [(n, bad, loss, c, x0) for n, bad in SIZES for loss, c in LOSSES for x0 in (False, True)]
BIG = (100, 30)                                                               # the accuracy scene: 100 matches, 30 displaced


@functools.lru_cache(maxsize=None)
def scene(n, n_bad, seed=None, focalL=50.0):
    seed = 7 * n + n_bad + 3 if seed is None else seed
    rng = np.random.default_rng(1000 + seed)
    C, CalM, Rt0, X = generate_scene_batch(1, n, noise=1.0, seed=seed, focalL=focalL)
    C = C[0].copy()
    bad = np.sort(rng.choice(n, n_bad, replace=False))
    C[bad] += rng.uniform(20.0, 80.0, (n_bad, 6)) * rng.choice([-1.0, 1.0], (n_bad, 6))
    sc = np.linalg.norm(Rt0[0][:, 3])
    truth = [np.hstack([Rt[:, :3], Rt[:, 3:4] / sc]) for Rt in Rt0]
    start = []
    for Rt in truth:
        k = rng.standard_normal(3); k /= np.linalg.norm(k); th = 0.02
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx) @ Rt[:, :3]
        start.append(np.hstack([R, Rt[:, 3:4] * (1 + 0.02 * rng.standard_normal((3, 1)))]))
    K, Ps, _, _ = scene_cameras(focalL)
    M1 = np.linalg.solve(K, Ps[0]); M1 = M1 / np.linalg.norm(M1[0, :3])         # [R1 | -R1 C1]: the points in the frame of camera 1
    X0 = (X[0] @ M1[:, :3].T + M1[:, 3]) / sc * (1 + 0.01 * rng.standard_normal((n, 3)))
    return dict(C=C, CalM=CalM, R_t_0=np.vstack([np.eye(3, 4)] + start), start=start, truth=truth, X0=X0, bad=bad)


@functools.lru_cache(maxsize=None)
def restated(n, n_bad, loss, c, with_x0, seed=None):
    """the restatement's run on a scene; left unchanged by its users"""
    sc = scene(n, n_bad, seed)
    return LO.ba_loss(sc["CalM"], sc["R_t_0"], sc["C"].T.copy(), sc["X0"].T.copy() if with_x0 else None, loss, c)


def rot_err_deg(R, Rt):
    c = (np.trace(R.T @ Rt[:, :3]) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def gate(ref, status, it, err, Rt2, Rt3, rec, weight, what):
    """the BA gate of tests/test_bundle_adjustment.py, with the weights: status 0, the same iter, repr_err, poses and points within 1e-9 relative, the
    weights within 1e-9 absolute.  Rt2, Rt3 3x4, rec 3xN."""
    rel = lambda a, r: np.abs(a - r).max() / np.abs(r).max()
    assert ref["margin"] >= 1e-10, (what, ref["margins"])                       # an iter that differs is then a defect and not a tie
    assert status == 0 and it == ref["iter"], (what, status, it, ref["iter"])
    assert abs(err - ref["repr_err"]) <= 1e-9 * ref["repr_err"] + 1e-12, (what, err, ref["repr_err"])
    assert rel(Rt2, ref["R_t"][3:6]) < 1e-9 and rel(Rt3, ref["R_t"][6:9]) < 1e-9, what
    assert rel(rec, ref["Reconst"]) < 1e-9, what
    assert np.abs(weight - ref["weight"]).max() <= 1e-9, what
