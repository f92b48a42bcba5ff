"""
TEST INFRASTRUCTURE ONLY -- the numpy restatement of the three-view bundle adjustment with a robust loss (include/tftfund_loss.h,
csrc/ba_kernel.h: k_bundle_adjust_loss).  The residual and Jacobian callback, the Euler angles and the constants are those of oracle/ba_oracle.py;
what is restated here is the Levenberg-Marquardt loop of that file with the loss added, statement by statement:

  * the pixel residual e_{i,v} = r_{i,v} / s_v (s_v: the isotropic scale of view v's Normalize2Ddata matrix), F = sum_i rho(|e_i|^2);
  * at the current parameters w_i = rho'(|e_i|^2); the residual rows of correspondence i in view v and the same rows of the Jacobian are multiplied
    by sqrt(w_i) / s_v, and the step is that of the plain loop on the scaled system (the weights of the current point, no second-order correction);
  * the step is then freed of its component along the scale gauge v = (0, t2, t3, X).  The cost does not change along v, so J v = 0, v . gradient = 0
    and the step of the loop has no such component; but in pixels only the damping, 1e-11 and less of the matrix, stands in that direction, and a
    dense solve leaves rounding noise of any size there (two orders of elimination moved the scale of the solution by 1e-4, the normalised poses
    by 1.5e-9, the weights by 1e-6).  step -= v (v . step) / (v . v) sets the component to its exact value; the kernel does the same;
  * the costs S and S_trial that steer acceptance and the function tolerance are sum rho(|e|^2), without frozen weights;
  * repr_err = sqrt(F) at the end, the weights w_i at the final parameters, the poses and points in the scale |t2| = 1.

loss None is least squares in the pixel metric (w = 1).  The run also returns the smallest relative margin by which each of its steering comparisons
-- S_trial < S, the function tolerance, the step tolerance -- was decided: a kernel that agrees with this file to 1e-9 takes the same decisions when
those margins are far above that.
"""
import numpy as np

from oracle import tft_oracle as O
from oracle.ba_oracle import bundleadjustment_LM, _rot_parts, _euler_angles, LM_INIT_DAMPING, LM_TOL_FUN, LM_TOL_X, LM_MAX_ITER


def rho(loss, c, s):
    if loss is None:
        return s
    if loss == "huber":
        return np.where(s <= c * c, s, 2.0 * c * np.sqrt(s) - c * c)
    if loss == "cauchy":
        return c * c * np.log1p(s / (c * c))
    raise ValueError(loss)


def rho1(loss, c, s):
    if loss is None:
        return np.ones_like(s)
    if loss == "huber":
        return np.where(s <= c * c, 1.0, c / np.sqrt(np.maximum(s, 1e-300)))
    if loss == "cauchy":
        return 1.0 / (1.0 + s / (c * c))
    raise ValueError(loss)


def prepare(CalM, R_t_0, Corresp, Reconst0=None):
    """BundleAdjustment.m:52-100 for three views with camera 1 = [I|0]: normalised points and calibration, the scales s_v, the variable vector"""
    CalM = CalM.copy(); Corresp = Corresp.copy()
    s = np.zeros(3)
    for j in range(3):
        Corresp[2 * j:2 * j + 2], Normal = O.Normalize2Ddata(Corresp[2 * j:2 * j + 2])
        CalM[3 * j:3 * j + 3] = Normal @ CalM[3 * j:3 * j + 3]
        s[j] = Normal[0, 0]
    if Reconst0 is None:
        X = O.triangulation3D([CalM[3 * j:3 * j + 3] @ R_t_0[3 * j:3 * j + 3] for j in range(3)], Corresp)
        Reconst0 = X[0:3] / X[3:4]
    assert np.array_equal(R_t_0[0:3], np.eye(3, 4))
    angles0 = np.stack([_euler_angles(R_t_0[3 * j:3 * j + 3, 0:3]) for j in (1, 2)], axis=1)
    trans0 = np.stack([R_t_0[3 * j:3 * j + 3, 3] for j in (1, 2)], axis=1)
    x0 = np.hstack([angles0, trans0, Reconst0]).reshape(-1, order='F')
    return x0, Corresp, CalM, s


def e2_of(F, s):
    """|e_i|^2 per correspondence from the normalised residual vector (six entries per correspondence, two per view)"""
    return ((F.reshape(-1, 3, 2) / s[None, :, None]) ** 2).sum(axis=(1, 2))


def cost_and_gradient(x, Corresp_n, CalM_n, s, loss, c):
    """F = sum rho(|e|^2) and its gradient 2 J' diag(rho' / s^2) r"""
    F, J = bundleadjustment_LM(x, Corresp_n, CalM_n, True)
    e2 = e2_of(F, s)
    row = (rho1(loss, c, e2)[:, None, None] / (s * s)[None, :, None] * np.ones((1, 1, 2))).reshape(-1)
    return float(rho(loss, c, e2).sum()), 2.0 * J.T @ (row * F)


def _margin(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def ba_loss(CalM, R_t_0, Corresp, Reconst0=None, loss=None, scale=None):
    """CalM 9x3, R_t_0 9x4 (camera 1 = [I|0]), Corresp 6xN, Reconst0 3xN or None.
    -> dict(R_t 9x4, Reconst 3xN, iter, repr_err, weight (N,), margins dict(accept, fun, step), margin = the smallest of them)"""
    c = None if loss is None else float(scale)
    x, Cn, Kn, s = prepare(CalM, R_t_0, Corresp, Reconst0)
    N = Corresp.shape[1]
    func = lambda v, jac: bundleadjustment_LM(v, Cn, Kn, jac)
    cost = lambda Fv: float(rho(loss, c, e2_of(Fv, s)).sum())

    def scaled(Fv, Jv):
        f = (np.sqrt(rho1(loss, c, e2_of(Fv, s)))[:, None, None] / s[None, :, None] * np.ones((1, 1, 2))).reshape(-1)
        Fw = f * Fv; Jw = f[:, None] * Jv
        return Jw.T @ Fw, Jw.T @ Jw

    lam = LM_INIT_DAMPING
    F, J = func(x, True)
    S = cost(F)
    g, H = scaled(F, J)
    it = 0
    margins = dict(accept=np.inf, fun=np.inf, step=np.inf)
    while it < LM_MAX_ITER:
        step = -np.linalg.solve(H + lam * np.eye(H.shape[0]), g)
        v = x.copy(); v[0:6] = 0.0                                          # the scale gauge (0, t2, t3, X): J v = 0, so the step has no component along it;
        step = step - v * ((v @ step) / (v @ v))                           # what rounding leaves there (the pivot is the damping alone) is taken out
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
            lam = lam / 10.0
            if done:
                break
        else:
            lam = lam * 10.0
            if small_step or lam > 1e16:
                break
    Ff = func(x, False)
    e2 = e2_of(Ff, s)
    v = x.reshape(3, N + 4, order='F')
    sc = 1.0 / np.linalg.norm(v[:, 2])
    R_t = np.zeros((9, 4)); R_t[0:3] = np.eye(3, 4)
    for j in range(2):
        Rx, Ry, Rz = _rot_parts(v[:, j])[0:3]
        R_t[3 * j + 3:3 * j + 6] = np.hstack([Rx @ Ry @ Rz, sc * v[:, 2 + j:3 + j]])
    return dict(R_t=R_t, Reconst=sc * v[:, 4:], iter=it, repr_err=float(np.sqrt(rho(loss, c, e2).sum())), weight=rho1(loss, c, e2), margins=margins,
                margin=min(margins.values()), x=x)
