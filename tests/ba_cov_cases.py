"""
TEST INFRASTRUCTURE ONLY -- the cases of the covariance tests (tests/test_emulated_ba_cov.py, tests/test_gpu_ba_cov.py): the scenes of
tests/ba_loss_cases.py, the restatement's own optimum on each (so that the kernel and tests/ba_cov_oracle.py see the same parameters), the restated
covariance there, and the gates.  Everything is computed once per process and left unchanged by its users.
"""
import functools

import numpy as np

import ba_cov_oracle as CO
import ba_loss_cases as bc
from oracle.ba_oracle import BundleAdjustment

# (matches, displaced): lane trips of one, one, one, two, and three with a remainder; 4 is the smallest count with a redundancy (3 m - 11 = 1)
SIZES = ((4, 0), (12, 0), (64, 8), (65, 13), (129, 0))
LOSSES = ((None, None), ("huber", 1.5), ("huber", 3.0), ("cauchy", 1.5), ("cauchy", 3.0))
CASES = [(n, bad, loss, c) for n, bad in SIZES for loss, c in LOSSES]
LOSS_ID = {None: 0, "huber": 1, "cauchy": 2}


@functools.lru_cache(maxsize=None)
def optimum(n, n_bad, loss, c, seed=None):
    """the restated adjustment's result from the scene's start: (R_t 9x4, Reconst 3xn) -- without a loss that of oracle/ba_oracle.py"""
    sc = bc.scene(n, n_bad, seed)
    if loss is None:
        R_t, X = BundleAdjustment(sc["CalM"], sc["R_t_0"], sc["C"].T.copy())[0:2]
    else:
        r = bc.restated(n, n_bad, loss, c, False, seed)
        R_t, X = r["R_t"], r["Reconst"]
    R_t.setflags(write=False); X.setflags(write=False)
    return R_t, X


@functools.lru_cache(maxsize=None)
def reference(n, n_bad, loss, c, seed=None):
    sc = bc.scene(n, n_bad, seed)
    R_t, X = optimum(n, n_bad, loss, c, seed)
    return CO.covariance(sc["CalM"], R_t, sc["C"].T.copy(), X, loss, c)


def biteq(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def gate(ref, cov, sigma0, point_cov, what):
    """cov 12x12, sigma0, point_cov (m, 6) against the restatement: cov and every point block within 1e-9 of the largest entry of the block (the
    project's BA gate; the restated routes differ by 5e-12), sigma0 within 1e-9 relative, cov symmetric TO THE BIT (the kernel symmetrises the
    inverse, and what follows is a product of commuting factors), and the gauge condition |cov h12| <= 1e-9 |cov| (h12 = (0, 0, t2, 0), |t2| = 1)."""
    figs = dict(cov=np.abs(cov - ref["cov"]).max() / np.abs(ref["cov"]).max(),
                point=(np.abs(point_cov - ref["point_cov"]).max(axis=1) / np.abs(ref["point_cov"]).max(axis=1)).max(),
                sigma0=abs(sigma0 - ref["sigma0"]) / ref["sigma0"],
                gauge=np.abs(cov @ ref["h12"]).max() / np.linalg.norm(cov, 2))
    print(what, figs)
    assert np.isfinite(cov).all() and np.isfinite(point_cov).all() and sigma0 > 0.0, what
    assert figs["cov"] <= 1e-9 and figs["point"] <= 1e-9 and figs["sigma0"] <= 1e-9, (what, figs)
    assert biteq(cov, cov.T), what
    assert figs["gauge"] <= 1e-9, (what, figs)
    assert np.linalg.eigvalsh(cov)[1] > 0.0, what                             # rank 11: one zero, eleven positive


def ragged_case():
    """a packed batch for the ragged chain: m = 0, 3, 4, 64, 65 selected out of larger ranges and a last item whose range ends beyond n_total.  The poses
    and points are each scene's start (the covariance is evaluated where it is asked for; the ragged contract is about bits)."""
    rng = np.random.default_rng(11)
    sizes = [10, 9, 12, 80, 90, 7]
    keep = [0, 3, 4, 64, 65, 7]
    scs = [bc.scene(n, min(3, n // 6), seed=70 + k, focalL=38.0 + 3.0 * k) for k, n in enumerate(sizes)]
    packed = np.ascontiguousarray(np.concatenate([s["C"] for s in scs]))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    nt = int(off[-1])
    off[-1] = nt + 5                                                            # the last item: bad offsets
    mask = np.concatenate([np.isin(np.arange(n), rng.choice(n, k, replace=False)) * rng.choice([1, 255]) for n, k in zip(sizes, keep)]).astype(np.uint8)
    cm = lambda Rt: np.ascontiguousarray(Rt.T).reshape(12)
    return dict(sizes=sizes, keep=keep, scs=scs, packed=packed, off=off, nt=nt, mask=mask,
                calms=np.ascontiguousarray(np.stack([s["CalM"].T.reshape(27) for s in scs])),
                r2=np.ascontiguousarray(np.stack([cm(s["start"][0]) for s in scs])), r3=np.ascontiguousarray(np.stack([cm(s["start"][1]) for s in scs])),
                X=np.ascontiguousarray(np.concatenate([s["X0"] for s in scs])))


def check_ragged(rc, mk, cov, sigma0, pc, fixed):
    """the outputs of a ragged call on ragged_case() (cov (B,144), sigma0 (B,), pc (nt + guard, 6), all preset to 5.0) against `fixed(b, sel)`, the fixed
    call with B = 1 on item b's selection -> (cov 144, sigma0, pc (m, 6)): valid items bit-equal, the others NaN, nothing else touched"""
    B, nt, off = len(rc["sizes"]), rc["nt"], rc["off"]
    assert (pc[nt:] == 5.0).all()
    for b in range(B):
        o0, o1 = int(off[b]), int(off[b + 1])
        if o1 > nt:                                                            # bad offsets: NaN, and no range to write to
            assert np.isnan(cov[b]).all() and np.isnan(sigma0[b]) and (pc[o0:nt] == 5.0).all(), b
            continue
        sel = mk[o0:o1] != 0 if mk is not None else np.ones(o1 - o0, dtype=bool)
        m = int(sel.sum())
        if m <= 3:
            assert np.isnan(cov[b]).all() and np.isnan(sigma0[b]) and np.isnan(pc[o0:o1]).all(), (b, m)
            continue
        fc, fs, fp = fixed(b, sel)
        assert np.isfinite(fc).all() and np.isfinite(fp).all() and fs > 0.0, b
        assert biteq(cov[b], fc) and biteq(sigma0[b:b + 1], np.array([fs])), b
        assert biteq(pc[o0:o1][sel], fp) and np.isnan(pc[o0:o1][~sel]).all(), b


# ---- Monte Carlo: is the predicted covariance the scatter of the result? ---------------------------------------------------------------------------------
MC_N, MC_SEED = 40, 7 * 40 + 2 + 3          # the generator seed of ba_loss_cases.scene(40, 2): the geometry of the N = 40 scene of the other BA tests


@functools.lru_cache(maxsize=None)
def mc_scene():
    """one scene of 40 matches without noise and its truth in the scale |t2| = 1 (poses 3x4, points (n, 3) in the frame of camera 1)"""
    from tft_vs_fund_amd.scenes import generate_scene_batch, scene_cameras
    C, CalM, Rt0, X = generate_scene_batch(1, MC_N, noise=0.0, seed=MC_SEED)
    sc = np.linalg.norm(Rt0[0][:, 3])
    truth = [np.hstack([Rt[:, :3], Rt[:, 3:4] / sc]) for Rt in Rt0]
    K, Ps, _, _ = scene_cameras()
    M1 = np.linalg.solve(K, Ps[0]); M1 = M1 / np.linalg.norm(M1[0, :3])
    return dict(C=C[0], CalM=CalM, truth=truth, R_t_0=np.vstack([np.eye(3, 4)] + truth), X=(X[0] @ M1[:, :3].T + M1[:, 3]) / sc)


def mc_draws(T, seed=1):
    """T x n x 6 matches: the noiseless ones plus 1 px of Gaussian noise per coordinate"""
    return mc_scene()["C"][None] + np.random.default_rng(seed).standard_normal((T, MC_N, 6))


def mc_params(Rt2, Rt3):
    """poses (T,3,4) -> the twelve parameters (T,12): angles2, angles3 (BundleAdjustment.m:92-94), t2, t3"""
    ang = lambda R: np.stack([-np.arctan2(R[:, 1, 2], R[:, 2, 2]), -np.arctan2(-R[:, 0, 2], np.hypot(R[:, 1, 2], R[:, 2, 2])), -np.arctan2(R[:, 0, 1], R[:, 0, 0])], axis=1)
    return np.concatenate([ang(Rt2), ang(Rt3), Rt2[:, :, 3], Rt3[:, :, 3]], axis=1)


def mc_ratio(params, cov):
    """the empirical standard deviation of each parameter over the mean predicted one: params (T,12), cov (T,12,12) -> (12,)"""
    return params.std(axis=0, ddof=1) / np.sqrt(np.diagonal(cov, axis1=1, axis2=2)).mean(axis=0)
