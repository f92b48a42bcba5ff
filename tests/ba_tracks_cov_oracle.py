"""
TEST INFRASTRUCTURE ONLY -- the numpy restatement of the covariance of the bundle adjustment over tracks (include/tftfund_tracks_cov.h states the
definition; the kernel is csrc/ba_tracks_cov_kernel.h: k_ba_tracks_cov).  It is tests/ba_cov_oracle.py for M = 2 .. 6 views with per-point visibility,
built on ba_tracks_loss_oracle.prepare (rules 1 - 5 of include/tftfund_tracks.h: visibility, dropped points, per-view normalisation over the view's own
observations, the change of coordinates to camera 1) and on oracle/ba_oracle.bundleadjustment_LM, whose rows of a missing observation are zero.

At x = (angles of cameras 2..M, translations of cameras 2..M, X_i of the points taking part) brought to the output scale |t2| = 1, with J and r what
the tracks kernels accumulate -- without a loss the per-view normalised residual, with one the pixel residual of observation (v, i), both rows times
sqrt(w_{v,i}) / s_v, w_{v,i} = rho'(|e_{v,i}|^2) per observation --:

    estimated   camera j >= 2 is estimated iff its view is seen; an unseen camera is a constant: its rows and columns of cov are 0 and it is in no gauge
                vector.  View 2 unseen: the scale rests on a quantity that was not estimated, everything is NaN.
    N = J'J     over the estimated parameters, singular along v = (0 for angles; t_j of the estimated cameras; X_i)
    h           the gradient of |t2| = 1: t2 in camera 2's translation slots
    Q           the top-left block of inv([[N, g], [g', 0]]), g = sqrt(alpha) h, alpha = trace(S) / (6 C_s), S the Schur complement of the point blocks
    dof         2 n_obs - (6 C_s + 3 m - 1);  sigma0^2 = r'r / dof;  cov = sigma0^2 Q_cameras (P x P, P = 6 (M - 1));
                point_cov_i = sigma0^2 x the 3 x 3 diagonal block of Q of point i (xx xy xz yy yz zz), NaN over a dropped point.

`covariance` is that definition, dense.  `routes` gives Q by the bordered inverse and by the Schur form the kernel evaluates (an unseen camera's
block of S gets a unit diagonal for the solve and is zeroed afterwards),
    Q_c = inv(S + alpha h_P h_P') - v_P v_P' / (alpha (h_P'v_P)^2),     Q_Xi = inv(V_i) + inv(V_i) B_i' Q_c B_i inv(V_i).
"""
import numpy as np

import ba_tracks_loss_oracle as TLO
import ba_tracks_oracle as TO
from ba_loss_oracle import rho1
from ba_cov_oracle import pack6
from oracle.ba_oracle import bundleadjustment_LM


def dof_of(n_obs, C_s, m):
    """2 n_obs residual rows, 6 C_s + 3 m parameters, one of them the scale"""
    return 2 * int(n_obs) - (6 * int(C_s) + 3 * int(m) - 1)


def system(CalM, R_t, Corresp, Reconst, loss=None, scale=None):
    """CalM 3M x 3, R_t 3M x 4 (first camera free, any common scale), Corresp 2M x N, Reconst 3 x N (a dropped point's column is not read)
    -> None where the definition gives NaN before any algebra, else dict(x at |t2| = 1, J, r (weighted), M, m, take, seen, n_obs)"""
    CalM = np.asarray(CalM, dtype=np.float64); R_t = np.asarray(R_t, dtype=np.float64); Corresp = np.asarray(Corresp, dtype=np.float64)
    M = Corresp.shape[0] // 2
    if not np.isfinite(R_t).all():
        return None
    p = TLO.prepare(CalM, R_t, Corresp, np.asarray(Reconst, dtype=np.float64))
    if p["status"] != TO.ST_OK or not p["seen"][1] or not np.isfinite(p["x0"]).all():
        return None
    m = p["used"]
    v = p["x0"].reshape(3, m + 2 * (M - 1), order="F").copy()
    v[:, M - 1:] = v[:, M - 1:] / np.linalg.norm(v[:, M - 1])
    x = v.reshape(-1, order="F")
    F, J = bundleadjustment_LM(x, p["Corresp_n"], p["CalM_n"], True)
    if loss is not None:
        f = np.repeat((np.sqrt(rho1(loss, float(scale), TLO.e2_of(F, p["s"]))) / p["s"][None, :]).reshape(-1), 2)
        F = f * F; J = f[:, None] * J
    return dict(x=x, J=J, r=F, M=M, m=m, take=p["take"], seen=p["seen"], n_obs=int(p["vis"].sum()))


def _layout(s):
    """-> P, est (P,) bool: the camera parameters that are estimated, v and h over the P + 3 m parameters"""
    M, x = s["M"], s["x"]
    C = M - 1; P = 6 * C
    est = np.zeros(P, dtype=bool)
    for j in range(C):
        if s["seen"][j + 1]:
            est[3 * j:3 * j + 3] = True; est[3 * C + 3 * j:3 * C + 3 * j + 3] = True
    v = x.copy(); v[:3 * C] = 0.0; v[:P][~est] = 0.0
    h = np.zeros_like(x); h[3 * C:3 * C + 3] = x[3 * C:3 * C + 3]
    return P, est, v, h


def _schur(Nm, P):
    A, Bc, Vd = Nm[:P, :P], Nm[:P, P:], Nm[P:, P:]
    m = Vd.shape[0] // 3
    Vi = [np.linalg.inv(Vd[3 * i:3 * i + 3, 3 * i:3 * i + 3]) for i in range(m)]
    S = A.copy()
    for i in range(m):
        Bi = Bc[:, 3 * i:3 * i + 3]
        S -= Bi @ Vi[i] @ Bi.T
    return S, Bc, Vi


def routes(s):
    """Q by the bordered inverse over the estimated parameters (the definition) and by the Schur form: two dicts(Qc P x P, Qx (m, 3, 3))"""
    P, est, v, h = _layout(s)
    m = s["m"]; n = P + 3 * m
    Nm = s["J"].T @ s["J"]
    S, Bc, Vi = _schur(Nm, P)
    C_s = int(est.sum()) // 6
    alpha = np.trace(S) / (6.0 * C_s)
    keep = np.concatenate([est, np.ones(3 * m, dtype=bool)])
    k = int(keep.sum())
    g = np.sqrt(alpha) * h[keep]
    K = np.zeros((k + 1, k + 1)); K[:k, :k] = Nm[np.ix_(keep, keep)]; K[:k, k] = g; K[k, :k] = g
    Q = np.zeros((n, n)); Q[np.ix_(keep, keep)] = np.linalg.inv(K)[:k, :k]
    bordered = dict(Qc=Q[:P, :P], Qx=np.stack([Q[P + 3 * i:P + 3 * i + 3, P + 3 * i:P + 3 * i + 3] for i in range(m)]))
    hP, vP = h[:P], v[:P]
    Ss = S.copy(); Ss[~est, ~est] = 1.0                                       # (an unseen camera's rows and columns of S are zero)
    Qc = np.linalg.inv(Ss + alpha * np.outer(hP, hP)) - np.outer(vP, vP) / (alpha * (hP @ vP) ** 2)
    Qc[~est, :] = 0.0; Qc[:, ~est] = 0.0
    Qx = np.stack([Vi[i] + Vi[i] @ Bc[:, 3 * i:3 * i + 3].T @ Qc @ Bc[:, 3 * i:3 * i + 3] @ Vi[i] for i in range(m)])
    return bordered, dict(Qc=Qc, Qx=Qx)


def _nan(M, N):
    P = 6 * (M - 1)
    return dict(cov=np.full((P, P), np.nan), sigma0=np.nan, point_cov=np.full((N, 6), np.nan), hP=None, est=None, dof=None)


def covariance(CalM, R_t, Corresp, Reconst, loss=None, scale=None, route=0):
    """the definition (route 0; 1: the Schur form): dict(cov P x P, sigma0, point_cov (N, 6) with NaN rows where dropped, hP, est (P,) bool, dof)"""
    Corresp = np.asarray(Corresp, dtype=np.float64)
    M, N = Corresp.shape[0] // 2, Corresp.shape[1]
    s = system(CalM, R_t, Corresp, Reconst, loss, scale)
    if s is None:
        return _nan(M, N)
    P, est, v, h = _layout(s)
    dof = dof_of(s["n_obs"], int(est.sum()) // 6, s["m"])
    if dof <= 0:
        return dict(_nan(M, N), dof=dof)
    q = routes(s)[route]
    s2 = float(s["r"] @ s["r"]) / dof
    pc = np.full((N, 6), np.nan)
    pc[s["take"]] = s2 * pack6(q["Qx"])
    out = dict(cov=s2 * q["Qc"], sigma0=float(np.sqrt(s2)), point_cov=pc, hP=h[:P].copy(), est=est, dof=dof)
    if not (np.isfinite(out["cov"]).all() and np.isfinite(out["sigma0"]) and np.isfinite(pc[s["take"]]).all()):
        return dict(_nan(M, N), dof=dof)
    return out
