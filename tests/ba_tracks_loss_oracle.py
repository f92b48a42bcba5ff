"""
TEST INFRASTRUCTURE ONLY -- the numpy restatement of the bundle adjustment over tracks with a robust loss (include/tftfund_tracks_loss.h states the
definition; the kernel is csrc/ba_tracks_loss_kernel.h).  It is the loop of tests/ba_loss_oracle.py on tests/ba_tracks_oracle.prepare (rules 1 - 5 of
include/tftfund_tracks.h: visibility, dropped points, per-view normalisation over the view's own observations, triangulation, change of coordinates) and on
oracle/ba_oracle.bundleadjustment_LM, whose rows of a missing observation are zero:

  1. the loss is PER OBSERVATION: e_{v,i} = r_{v,i} / s_v (s_v the isotropic scale of view v's normalisation, 1 for an unseen view),
     F = sum over the observations that exist of rho(|e_{v,i}|^2); rho, rho' are those of tests/ba_loss_oracle.py;
  2. at the current parameters w_{v,i} = rho'(|e_{v,i}|^2); the two rows of observation (v, i) of the residual and of the Jacobian are multiplied by
     sqrt(w_{v,i}) / s_v; the step is that of the plain loop on the scaled system (no second-order term);
  3. the step is freed of its component along v = (0 for all angles; t_j of every camera that is seen; X_i of every point taking part);
  4. the dense system stands for the Schur system solved without a pivot floor;
  5. after a successful step lambda = max(lambda / 10, 1e-3); everything else is the plain loop;
  6. the steering costs are F at the current and at the trial parameters; repr_err = sqrt(F) at the end; the scale |t2| = 1;
  7. weight (N, M): w_{v,i} at the final parameters where the observation exists and the point takes part, NaN elsewhere and over a failed item.

The run returns the steering margins as tests/ba_loss_oracle.py does and, per system solved, whether a Cholesky factorisation of it succeeds.  `perm`
permutes the elimination order of the dense solve (the result must not depend on it beyond rounding).
"""
import numpy as np

import ba_tracks_oracle as TO
from ba_loss_oracle import rho, rho1, _margin
from oracle import tft_oracle as O
from oracle.ba_oracle import bundleadjustment_LM, _rot_parts, LM_INIT_DAMPING, LM_TOL_FUN, LM_TOL_X, LM_MAX_ITER

ST_OK = TO.ST_OK
LAMBDA_FLOOR = 1e-3


def prepare(CalM, R_t_0, Corresp, Reconst0=None):
    """ba_tracks_oracle.prepare plus s (M,): the scale of every view's normalisation (1: unseen) and seen (M,) bool"""
    p = TO.prepare(CalM, R_t_0, Corresp, Reconst0)
    if p["status"] != ST_OK:
        return p
    M = Corresp.shape[0] // 2
    C = Corresp[:, p["take"]]
    vis = TO.visibility(C)
    s = np.ones(M)
    for v in range(M):
        if vis[v].any():
            s[v] = O.Normalize2Ddata(C[2 * v:2 * v + 2, vis[v]])[1][0, 0]
    p.update(s=s, seen=vis.any(axis=1), vis=vis)
    return p


def e2_of(F, s):
    """|e_{v,i}|^2, (used, M), from the normalised residual vector (2M entries per point, two per view; zero where there is no observation)"""
    M = s.size
    return ((F.reshape(-1, M, 2) / s[None, :, None]) ** 2).sum(axis=2)


def cost_and_gradient(x, Corresp_n, CalM_n, s, loss, c):
    """F = sum rho(|e|^2) and its gradient 2 J' diag(rho' / s^2) r"""
    F, J = bundleadjustment_LM(x, Corresp_n, CalM_n, True)
    e2 = e2_of(F, s)
    row = np.repeat((rho1(loss, c, e2) / (s * s)[None, :]).reshape(-1), 2)
    return float(rho(loss, c, e2).sum()), 2.0 * J.T @ (row * F)


def gauge(x, M, seen):
    """rule 3: 0 for all angles, t_j for every camera that is seen, X_i for every point (x holds the points taking part only)"""
    v = x.copy()
    v[0:3 * (M - 1)] = 0.0
    for j in range(1, M):
        if not seen[j]:
            v[3 * (M - 1) + 3 * (j - 1):3 * (M - 1) + 3 * j] = 0.0
    return v


def ba_tracks_loss(CalM, R_t_0, Corresp, Reconst0=None, loss=None, scale=None, perm=None):
    """CalM 3M x 3, R_t_0 3M x 4, Corresp 2M x N (non-finite = not seen), Reconst0 3 x N or None; loss None | "huber" | "cauchy", scale in pixels.
    -> dict(R_t, Reconst (NaN columns where dropped), iter, repr_err, used, status, weight (N, M), margins, margin, chol (one bool per system solved))"""
    CalM = np.asarray(CalM, dtype=np.float64); R_t_0 = np.asarray(R_t_0, dtype=np.float64); Corresp = np.asarray(Corresp, dtype=np.float64)
    M, N = Corresp.shape[0] // 2, Corresp.shape[1]
    c = None if loss is None else float(scale)
    p = prepare(CalM, R_t_0, Corresp, Reconst0)
    if p["status"] != ST_OK:
        return dict(R_t=np.full((3 * M, 4), np.nan), Reconst=np.full((3, N), np.nan), iter=0, repr_err=np.nan, used=p["used"], status=p["status"],
                    weight=np.full((N, M), np.nan), margins={}, margin=np.inf, chol=[])
    Cn, Kn, s, seen, x = p["Corresp_n"], p["CalM_n"], p["s"], p["seen"], p["x0"].copy()
    func = lambda v, jac: bundleadjustment_LM(v, Cn, Kn, jac)
    cost = lambda Fv: float(rho(loss, c, e2_of(Fv, s)).sum())

    def scaled(Fv, Jv):
        f = np.repeat((np.sqrt(rho1(loss, c, e2_of(Fv, s))) / s[None, :]).reshape(-1), 2)
        Fw = f * Fv; Jw = f[:, None] * Jv
        return Jw.T @ Fw, Jw.T @ Jw

    lam = LM_INIT_DAMPING
    F, J = func(x, True)
    S = cost(F)
    g, H = scaled(F, J)
    n = x.size
    q = np.arange(n) if perm is None else np.asarray(perm)
    it = 0
    margins = dict(accept=np.inf, fun=np.inf, step=np.inf)
    chol = []
    while it < LM_MAX_ITER:
        A = H + lam * np.eye(n)
        try:
            np.linalg.cholesky(A); chol.append(True)
        except np.linalg.LinAlgError:
            chol.append(False)
        step = np.zeros(n)
        step[q] = -np.linalg.solve(A[np.ix_(q, q)], g[q])
        v = gauge(x, M, seen)                                               # rule 3
        step = step - v * ((v @ step) / (v @ v))
        St = cost(func(x + step, False))
        thr = LM_TOL_X * (np.sqrt(np.finfo(float).eps) + np.linalg.norm(x))
        small_step = np.linalg.norm(step) < thr
        margins["step"] = min(margins["step"], _margin(np.linalg.norm(step), thr))
        margins["accept"] = min(margins["accept"], _margin(St, S))
        if St < S:
            x = x + step
            it += 1
            margins["fun"] = min(margins["fun"], _margin(abs(St - S), LM_TOL_FUN * S))
            done = abs(St - S) <= LM_TOL_FUN * S or small_step
            F, J = func(x, True)
            S = cost(F)
            g, H = scaled(F, J)
            lam = max(lam / 10.0, LAMBDA_FLOOR)                             # rule 5
            if done:
                break
        else:
            lam = lam * 10.0
            if small_step or lam > 1e16:
                break
    e2 = e2_of(func(x, False), s)
    vv = x.reshape(3, p["used"] + 2 * (M - 1), order="F")
    angles, trans = vv[:, 0:M - 1], vv[:, M - 1:2 * (M - 1)]
    sc = 1.0 / np.linalg.norm(trans[:, 0])
    R_t = np.zeros((3 * M, 4)); R_t[0:3] = np.eye(3, 4)
    for j in range(M - 1):
        Rx, Ry, Rz = _rot_parts(angles[:, j])[0:3]
        R_t[3 * j + 3:3 * j + 6] = np.hstack([Rx @ Ry @ Rz, sc * trans[:, j:j + 1]])
    Reconst = np.full((3, N), np.nan)
    Reconst[:, p["take"]] = sc * vv[:, 2 * (M - 1):]
    weight = np.full((N, M), np.nan)
    w = rho1(loss, c, e2)
    w = np.where(p["vis"].T, w, np.nan)
    weight[p["take"]] = w
    return dict(R_t=R_t, Reconst=Reconst, iter=it, repr_err=float(np.sqrt(rho(loss, c, e2).sum())), used=p["used"], status=ST_OK, weight=weight,
                margins=margins, margin=min(margins.values()), chol=chol, x=x, prep=p)
