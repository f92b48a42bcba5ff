"""
TEST INFRASTRUCTURE ONLY -- the numpy restatement of the bundle adjustment over tracks (include/tftfund_tracks.h states the definition; the kernel is
csrc/ba_tracks_kernel.h).  BundleAdjustment.m:4-22 documents per-point visibility ("If point n is not seen in image m, then Corresp(2*m-1:2*m,n)=[NaN;NaN]")
and its code cannot do it; this is the documented behaviour, built from the pieces of the restated reference: oracle.ba_oracle.bundleadjustment_LM (the
callback, whose `isnan` branch leaves the rows of a missing observation zero), levenberg_marquardt, _euler_angles and oracle.tft_oracle.triangulation3D.

  1. observation (v, i) exists iff both coordinates are finite;
  2. a point takes part iff it has >= 2 observations; every other point is dropped before everything else and comes back as a NaN column;
  3. view v is normalised (Normalize2Ddata.m:33-39) over its n_v observations of points taking part; n_v = 0: unseen, the camera keeps its start;
     n_v >= 1 and a normalisation that is not finite: ST_NONFINITE, NaN everywhere;
  4. no point taking part: ST_TOO_FEW, NaN everywhere;
  5. triangulation from the views that see the point (:59-77), change of coordinates, angles, variables (:80-100), callback (:128-204);
  6. the LM loop of oracle/ba_oracle.py over all camera parameters and the points taking part;
  7. R_t(1:3,:) = eye(3,4), scale 1/|t2|, repr_err = |f| over the observations that exist.
"""
import numpy as np

from oracle import ba_oracle as BA
from oracle import tft_oracle as O

ST_OK, ST_TOO_FEW, ST_NONFINITE = 0, 1, 2


def visibility(Corresp):
    """(M, N) bool: observation (v, i) exists (rule 1)"""
    return np.isfinite(Corresp[0::2]) & np.isfinite(Corresp[1::2])


def prepare(CalM, R_t_0, Corresp, Reconst0=None):
    """Rules 1-5 up to the variable vector.  -> dict(status, used, take) and, for status 0, x0, Corresp_n (2M x used, NaN where not seen), CalM_n."""
    M = Corresp.shape[0] // 2
    vis = visibility(Corresp)
    take = vis.sum(axis=0) >= 2                                                          # rule 2
    used = int(take.sum())
    if used == 0:                                                                        # rule 4
        return dict(status=ST_TOO_FEW, used=0, take=take)
    C = Corresp[:, take].copy(); vis = vis[:, take]
    C[np.repeat(~vis, 2, axis=0)] = np.nan                                               # (an Inf, or a finite partner of a NaN: not seen, :165 tests the x row)
    K = CalM.copy()
    seen = vis.any(axis=1)
    for v in range(M):                                                                   # rule 3
        if not seen[v]:
            continue
        with np.errstate(all="ignore"):
            pts, Normal = O.Normalize2Ddata(C[2 * v:2 * v + 2, vis[v]])
        if not np.isfinite(Normal).all():
            return dict(status=ST_NONFINITE, used=used, take=take)
        C[2 * v:2 * v + 2, vis[v]] = pts
        K[3 * v:3 * v + 3] = Normal @ K[3 * v:3 * v + 3]
    R0 = R_t_0.copy()
    if Reconst0 is None:                                                                 # rule 5: :59-77, the views that see the point
        X0 = np.zeros((3, used))
        for i in range(used):
            js = np.flatnonzero(vis[:, i])
            X = O.triangulation3D([K[3 * j:3 * j + 3] @ R0[3 * j:3 * j + 3] for j in js], np.concatenate([C[2 * j:2 * j + 2, i:i + 1] for j in js]))
            X0[:, i] = X[0:3, 0] / X[3, 0]
    else:
        X0 = Reconst0[:, take].copy()
    cc = R0[0:3].copy()                                                                  # :80-86
    R0[0:3] = np.eye(3, 4)
    for j in range(1, M):
        R0[3 * j:3 * j + 3, 3] = R0[3 * j:3 * j + 3, 3] - R0[3 * j:3 * j + 3, 0:3] @ cc[:, 0:3].T @ cc[:, 3]
        R0[3 * j:3 * j + 3, 0:3] = R0[3 * j:3 * j + 3, 0:3] @ cc[:, 0:3].T
    X0 = cc[:, 0:3] @ X0 + cc[:, 3:4]
    angles0 = np.stack([BA._euler_angles(R0[3 * j:3 * j + 3, 0:3]) for j in range(1, M)], axis=1)          # :89-96
    trans0 = np.stack([R0[3 * j:3 * j + 3, 3] for j in range(1, M)], axis=1)
    x0 = np.hstack([angles0, trans0, X0]).reshape(-1, order="F")                         # :100
    return dict(status=ST_OK, used=used, take=take, x0=x0, Corresp_n=C, CalM_n=K)


def BundleAdjustmentTracks(CalM, R_t_0, Corresp, Reconst0=None, return_debug=False):
    """-> R_t (3M x 4), Reconst (3 x N, NaN columns where dropped), iter, repr_err, used, status"""
    CalM = np.asarray(CalM, dtype=np.float64); R_t_0 = np.asarray(R_t_0, dtype=np.float64); Corresp = np.asarray(Corresp, dtype=np.float64)
    M, N = Corresp.shape[0] // 2, Corresp.shape[1]
    p = prepare(CalM, R_t_0, Corresp, Reconst0)
    if p["status"] != ST_OK:
        out = (np.full((3 * M, 4), np.nan), np.full((3, N), np.nan), 0, np.nan, p["used"], p["status"])
        return out + (p,) if return_debug else out
    func = lambda x, jac: BA.bundleadjustment_LM(x, p["Corresp_n"], p["CalM_n"], jac)
    x, it, evals = BA.levenberg_marquardt(func, p["x0"])                                 # rule 6
    repr_err = float(np.linalg.norm(func(x, False)))                                     # rule 7
    v = x.reshape(3, p["used"] + 2 * (M - 1), order="F")
    angles, trans = v[:, 0:M - 1], v[:, M - 1:2 * (M - 1)]
    scale = 1.0 / np.linalg.norm(trans[:, 0])
    R_t = np.zeros((3 * M, 4)); R_t[0:3] = np.eye(3, 4)
    for j in range(M - 1):
        Rx, Ry, Rz = BA._rot_parts(angles[:, j])[0:3]
        R_t[3 * j + 3:3 * j + 6] = np.hstack([Rx @ Ry @ Rz, scale * trans[:, j:j + 1]])
    Reconst = np.full((3, N), np.nan)
    Reconst[:, p["take"]] = scale * v[:, 2 * (M - 1):]
    out = (R_t, Reconst, it, repr_err, p["used"], ST_OK)
    if return_debug:
        p.update(x=x, evals=evals, cost0=float(np.linalg.norm(func(p["x0"], False))))
        return out + (p,)
    return out


def check_jacobian_and_optimum(CalM, R_t_0, Corresp, Reconst0=None, n_cols=12, seed=1):
    """What test_oracle_jacobian_and_converged_optimum (tests/test_bundle_adjustment.py) does for the full case, on a partially visible one: the analytic
    Jacobian of the callback against central differences in `n_cols` random variables, and the optimum of the LM loop against MINPACK's (scipy) to the
    FunctionTolerance.  Returns (largest Jacobian deviation, |err - err_minpack| / err)."""
    from scipy.optimize import least_squares
    R_t, Rec, it, err, used, st, d = BundleAdjustmentTracks(CalM, R_t_0, Corresp, Reconst0, True)
    assert st == ST_OK
    fun = lambda x: BA.bundleadjustment_LM(x, d["Corresp_n"], d["CalM_n"], False)
    f, J = BA.bundleadjustment_LM(d["x0"], d["Corresp_n"], d["CalM_n"])
    h, worst = 1e-6, 0.0
    for k in np.random.default_rng(seed).integers(0, d["x0"].size, n_cols):
        e = np.zeros(d["x0"].size); e[k] = h
        worst = max(worst, float(np.abs((fun(d["x0"] + e) - fun(d["x0"] - e)) / (2 * h) - J[:, k]).max()))
    missing = ~np.isfinite(d["Corresp_n"]).reshape(-1, order="F")
    assert missing.any() and not f[missing].any() and not J[missing].any()               # zero rows where there is no observation
    sol = least_squares(fun, d["x0"], jac=lambda x: BA.bundleadjustment_LM(x, d["Corresp_n"], d["CalM_n"])[1], method="lm", xtol=1e-13, ftol=1e-13)
    assert err <= d["cost0"]
    return worst, abs(err - float(np.linalg.norm(sol.fun))) / err
