"""
TEST INFRASTRUCTURE ONLY -- the numpy restatement of the covariance of the three-view bundle adjustment (include/tftfund_cov.h,
csrc/ba_cov_kernel.h: k_ba_cov), built on the residual / Jacobian callback of oracle/ba_oracle.py and the losses of tests/ba_loss_oracle.py.

At the parameters x = (angles2, angles3, t2, t3, X_1 .. X_m) (BundleAdjustment.m:100) brought to the output scale |t2| = 1, with J and r the Jacobian
and the residual the kernel accumulates -- without a loss the per-view normalised residual; with one the pixel residual, its rows times
sqrt(w_i) / s_v, w_i = rho'(|e_i|^2) --:

    N = J'J                      singular along the scale gauge v = (0, 0, t2, t3, X)
    h = (0, 0, t2, 0, 0 ..)      the gradient of the gauge |t2| = 1 the output is in
    Q                            the cofactor matrix: the top-left block of inv([[N, g], [g', 0]]), g = sqrt(alpha) h, alpha = trace(S) / 12 with S the
                                 Schur complement of the point blocks of N (the border of an exact inverse may have any length; this one keeps the
                                 bordered matrix as well conditioned as N's own range: in pixels N is 1e8 and a border of length 1 costs eight digits)
    sigma0^2 = r'r / (3 m - 11)  6 m residuals, 11 + 3 m free parameters
    cov = sigma0^2 Q[0:12, 0:12],    point_cov_i = sigma0^2 Q[12 + 3 i : 15 + 3 i, 12 + 3 i : 15 + 3 i]  (packed xx xy xz yy yz zz)

`covariance` is that definition, dense.  `routes` gives Q three ways -- the bordered inverse, the projected pseudo-inverse P N^+ P' with
P = I - v h' / (h'v), and the Schur form the kernel evaluates,
    Q_c = inv(S + alpha h12 h12') - v12 v12' / (alpha (h12'v12)^2),     Q_Xi = inv(V_i) + inv(V_i) B_i' Q_c B_i inv(V_i)
-- for tests/test_ba_cov_cpu.py to compare.
"""
import numpy as np

import ba_loss_oracle as LO
from oracle.ba_oracle import bundleadjustment_LM, _rot_parts


def system(CalM, R_t, Corresp, Reconst, loss=None, scale=None):
    """CalM 9x3, R_t 9x4 (camera 1 = [I|0]), Corresp 6xN, Reconst 3xN -> x at |t2| = 1, the weighted J and r, m"""
    x, Cn, Kn, s = LO.prepare(CalM, R_t, Corresp, Reconst)
    m = Corresp.shape[1]
    v = x.reshape(3, m + 4, order='F').copy()
    v[:, 2:] = v[:, 2:] / np.linalg.norm(v[:, 2])
    x = v.reshape(-1, order='F')
    F, J = bundleadjustment_LM(x, Cn, Kn, True)
    if loss is not None:
        f = (np.sqrt(LO.rho1(loss, float(scale), LO.e2_of(F, s)))[:, None, None] / s[None, :, None] * np.ones((1, 1, 2))).reshape(-1)
        F = f * F; J = f[:, None] * J
    return x, J, F, m


def _gauge(x):
    v = x.copy(); v[0:6] = 0.0
    h = np.zeros_like(x); h[6:9] = x[6:9]
    return v, h


def _schur(Nm):
    A, Bc, Vd = Nm[:12, :12], Nm[:12, 12:], Nm[12:, 12:]
    m = Vd.shape[0] // 3
    Vi = [np.linalg.inv(Vd[3 * i:3 * i + 3, 3 * i:3 * i + 3]) for i in range(m)]
    S = A.copy()
    for i in range(m):
        Bi = Bc[:, 3 * i:3 * i + 3]
        S -= Bi @ Vi[i] @ Bi.T
    return S, Bc, Vi


def routes(x, J):
    """Q by the bordered inverse, the projected pseudo-inverse and the Schur form: three dicts(Qc 12x12, Qx (m,3,3))"""
    n = x.shape[0]; m = (n - 12) // 3
    Nm = J.T @ J
    v, h = _gauge(x)
    S, Bc, Vi = _schur(Nm)
    alpha = np.trace(S) / 12.0
    blocks = lambda Q: dict(Qc=Q[:12, :12], Qx=np.stack([Q[12 + 3 * i:15 + 3 * i, 12 + 3 * i:15 + 3 * i] for i in range(m)]))
    g = np.sqrt(alpha) * h
    K = np.zeros((n + 1, n + 1)); K[:n, :n] = Nm; K[:n, n] = g; K[n, :n] = g
    bordered = blocks(np.linalg.inv(K)[:n, :n])
    P = np.eye(n) - np.outer(v, h) / (h @ v)
    projected = blocks(P @ np.linalg.pinv(Nm, rcond=1e-13, hermitian=True) @ P.T)
    h12, v12 = h[:12], v[:12]
    Qc = np.linalg.inv(S + alpha * np.outer(h12, h12)) - np.outer(v12, v12) / (alpha * (h12 @ v12) ** 2)
    Qx = np.stack([Vi[i] + Vi[i] @ Bc[:, 3 * i:3 * i + 3].T @ Qc @ Bc[:, 3 * i:3 * i + 3] @ Vi[i] for i in range(m)])
    return bordered, projected, dict(Qc=Qc, Qx=Qx)


def pack6(Qx):
    return np.stack([Qx[:, 0, 0], Qx[:, 0, 1], Qx[:, 0, 2], Qx[:, 1, 1], Qx[:, 1, 2], Qx[:, 2, 2]], axis=1)


def covariance(CalM, R_t, Corresp, Reconst, loss=None, scale=None):
    """the definition: dict(cov 12x12, sigma0, point_cov (m, 6), h12) -- all NaN for m <= 3"""
    m = Corresp.shape[1]
    if m <= 3:
        return dict(cov=np.full((12, 12), np.nan), sigma0=np.nan, point_cov=np.full((m, 6), np.nan), h12=None)
    x, J, F, m = system(CalM, R_t, Corresp, Reconst, loss, scale)
    q = routes(x, J)[0]
    s2 = float(F @ F) / (3 * m - 11)
    return dict(cov=s2 * q["Qc"], sigma0=np.sqrt(s2), point_cov=s2 * pack6(q["Qx"]), h12=_gauge(x)[1][:12])


def pose_of(x):
    """the variable vector -> R_t 9x4 (as the adjustment writes it, without rescaling) and the points 3xm"""
    v = x.reshape(3, -1, order='F')
    R_t = np.zeros((9, 4)); R_t[0:3] = np.eye(3, 4)
    for j in range(2):
        Rx, Ry, Rz = _rot_parts(v[:, j])[0:3]
        R_t[3 * j + 3:3 * j + 6] = np.hstack([Rx @ Ry @ Rz, v[:, 2 + j:3 + j]])
    return R_t, v[:, 4:].copy()
