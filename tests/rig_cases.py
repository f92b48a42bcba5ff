"""
Inputs the rest of the suite does not have: a calibration matrix of its own for every view, and camera rigs other than the generator's.

tft_vs_fund_amd/scenes.py draws every scene from one K (CalM = [K; K; K], zero skew, K(3,3) = 1) and one rig (three converging cameras): with
K1 = K2 = K3 an index slip between the views of CalM changes no bit of any output.  The cases here are generated from a seed at run time:

  per_view_K(k)    three upper-triangular matrices with different focal lengths, principal points, skews of either sign and an overall scale each
                   (so K(3,3) != 1), different for every item index k;
  rig(name)        (R_v, C_v) per view with the first camera [I|0]: x_v ~ K_v R_v (X - C_v);
  rig_batch(...)   B scenes of N correspondences seen by that rig through those calibrations, with noise in pixels;
  swap_views_23    the control calibration: K2 and K3 exchanged.  A test that passes with it cannot see a view mix-up.

Plain module, no GPU; used by tests/test_gpu_rigs.py and tests/test_emulated_rigs.py.
"""
import numpy as np

from tft_vs_fund_amd.scenes import _rotation, scene_cameras

RIGS = ["converging", "parallel", "forward", "roll", "collinear_parallel"]
MIN_PARALLAX = 0.01        # radians: 20 pixels at a focal length of 2000, forty times the noise of the cases


def per_view_K(k=0):
    """(K1, K2, K3) for item index k: focal lengths 2000 / 2600 / 3300 (pairwise more than 20 % apart) times (1 + k / 100), fy = 1.02 fx, principal
    points that differ between the views and move with k, skews 3.5 / -6 / 9, and the whole matrix of view v scaled by 1.3 / 1.7 / 0.6."""
    k = int(k)
    g = 1.0 + 0.01 * k
    spec = [(2000.0, 900.0 + 7 * k, 600.0 - 5 * k, 3.5, 1.3), (2600.0, 820.0 - 4 * k, 660.0 + 3 * k, -6.0, 1.7), (3300.0, 1010.0 + 2 * k, 540.0 + 6 * k, 9.0, 0.6)]
    return [s * np.array([[f * g, skew, cx], [0.0, 1.02 * f * g, cy], [0.0, 0.0, 1.0]]) for f, cx, cy, skew, s in spec]


def calm_of(Ks):
    return np.vstack(Ks)


def per_view_calm(B=None):
    """CalM (9, 3) of item 0, or (B, 9, 3) with item k from per_view_K(k): no two items share a block."""
    if B is None:
        return calm_of(per_view_K(0))
    return np.stack([calm_of(per_view_K(k)) for k in range(B)])


def swap_views_23(CalM):
    """CalM (..., 3M, 3) with the blocks of views 2 and 3 exchanged."""
    out = np.array(CalM, dtype=float, copy=True)
    out[..., 3:6, :] = np.asarray(CalM)[..., 6:9, :]
    out[..., 6:9, :] = np.asarray(CalM)[..., 3:6, :]
    return out


def first_view_only(CalM):
    """CalM (..., 9, 3) -> [K1; K1; K1]"""
    out = np.array(CalM, dtype=float, copy=True)
    out[..., 3:6, :] = out[..., 0:3, :]
    out[..., 6:9, :] = out[..., 0:3, :]
    return out


def _rz(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def _ry(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def _generator_rig(angle=None):
    """the generator's three cameras (centres on one side of the point cube, every camera looking at its middle) in the frame of the first one"""
    if angle is None:
        p = 0.0
    else:
        a = angle * np.pi / 180.0
        p = 1 - np.sin(a) / (np.sqrt(2) * (np.cos(a) - 1))
    Cs = [np.array([0., -1400, 400]) + p * np.array([0., 300, -300]), np.array([-400., -1000, 0]) + p * np.array([0., -100, 100]),
          np.array([600., -800, -200]) + p * np.array([0., -300, 300])]
    down = np.array([0., 0, -1])
    Rs = [_rotation(c, down) for c in Cs]                                   # (R takes the centre's direction to -z: the cube's middle has depth +|C|)
    return [(R @ Rs[0].T, Rs[0] @ (c - Cs[0])) for R, c in zip(Rs, Cs)]


def rig(name):
    """[(R_1, C_1), (R_2, C_2), (R_3, C_3)] with (R_1, C_1) = (I, 0).
    converging            the generator's centres and look-at rotations
    converging_collinear  the same with the centres moved onto one line (the generator's angle = 180), for PiColPoseEstimation
    parallel              three parallel optical axes, centres in the plane z = 0: all epipoles at infinity
    forward               view 2 moved 250 along its own optical axis (the epipole of view 1 in image 2 is its principal point) and turned by 8
                          degrees about y; view 3 further ahead and as far aside as the other rigs' baselines.  (Without the turn, R2 = I and
                          t2 || z, the slice T(:,:,3) = a3 b4' - a4 b3' of the tensor has a3 || a4 and rank 1: R_t_from_TFT takes the epipoles from
                          the null vectors of the slices, and kernel and LAPACK oracle, which agree on T to 2e-14, then agree on R_t_3 only to
                          2e-10 .. 1e-9 -- the input is ill-posed for the reference's algorithm, not a case for a 1e-9 gate.)
    roll                  view 2 rolled by 100 degrees about its optical axis, view 3 by 180
    collinear_parallel    parallel axes and the three centres on one line in the plane z = 0"""
    I, z = np.eye(3), np.zeros(3)
    if name == "converging":
        return _generator_rig()
    if name == "converging_collinear":
        return _generator_rig(180.0)
    if name == "parallel":
        return [(I, z), (I, np.array([300.0, 40.0, 0.0])), (I, np.array([-120.0, 260.0, 0.0]))]
    if name == "forward":
        R2 = _ry(8.0)
        return [(I, z), (R2, R2.T @ np.array([0.0, 0.0, 250.0])), (I, np.array([240.0, -160.0, 450.0]))]
    if name == "roll":
        return [(I, z), (_rz(100.0), np.array([300.0, 50.0, 40.0])), (_rz(180.0), np.array([-200.0, 250.0, -60.0]))]
    if name == "collinear_parallel":
        return [(I, z), (I, np.array([250.0, 100.0, 0.0])), (I, np.array([550.0, 220.0, 0.0]))]
    raise ValueError("unknown rig %r" % (name,))


def _generator_calm():
    return scene_cameras()[3]


def rig_batch(name, B, N, noise, seed, K="per_view"):
    """B scenes of N correspondences of rig `name`.
    K: "per_view" -> CalM (B, 9, 3), item k calibrated by per_view_K(k); "shared" -> CalM (9, 3) = per_view_K(0) for every item;
       "generator" -> the generator's CalM (9, 3), three equal blocks.
    Points: uniform in the box |x| <= 500, |y| <= 350, 1200 <= z <= 2200 of the first camera's frame -- its near face fills the 1800 x 1200 image of
    the first camera (focal length 2000), and it lies in front of every camera of every rig (the baselines are a few hundred).  A point is redrawn
    when its two rays from view 1 and from view 2 or 3 meet at less than MIN_PARALLAX: the reference scales t3 through a triangulation from views 1
    and 2 alone (R_t_from_TFT.m:68-74), which is singular on the line through their centres -- in the forward rig that line crosses the box.  Noise: normal, `noise` pixels per coordinate (pixels = homogeneous image point divided by its third entry, whatever K(3,3) is).
    Returns Corresp (B, N, 6) C-contiguous, CalM, R_t_2, R_t_3 (3, 4) ground truth up to the scale of the translations, points (B, N, 3)."""
    cams = rig(name)
    if isinstance(K, str):
        CalM = {"per_view": lambda: per_view_calm(B), "shared": lambda: per_view_calm(), "generator": _generator_calm}[K]()
    else:
        CalM = np.asarray(K, dtype=float)
    rng = np.random.Generator(np.random.Philox(key=int(seed)))
    X = np.empty((B, N, 3))
    for b in range(B):
        have = 0
        while have < N:
            Xn = np.stack([rng.uniform(-500.0, 500.0, 2 * N), rng.uniform(-350.0, 350.0, 2 * N), rng.uniform(1200.0, 2200.0, 2 * N)], axis=1)
            keep = np.ones(2 * N, dtype=bool)
            for _, Cv in cams[1:]:                                            # parallax between view 1 and view v
                r1, rv = Xn, Xn - Cv
                cosang = np.sum(r1 * rv, axis=1) / (np.linalg.norm(r1, axis=1) * np.linalg.norm(rv, axis=1))
                keep &= np.arccos(np.clip(cosang, -1.0, 1.0)) >= MIN_PARALLAX
            Xn = Xn[keep][:N - have]
            X[b, have:have + Xn.shape[0]] = Xn
            have += Xn.shape[0]
    Corresp = np.empty((B, N, 6))
    for b in range(B):
        Kb = CalM[b] if CalM.ndim == 3 else CalM
        for v, (R, C) in enumerate(cams):
            xc = (X[b] - C) @ R.T
            assert xc[:, 2].min() > 100.0, "a point behind or too close to camera %d of rig %s" % (v + 1, name)
            xh = xc @ Kb[3 * v:3 * v + 3].T
            Corresp[b, :, 2 * v:2 * v + 2] = xh[:, 0:2] / xh[:, 2:3]
    Corresp += noise * rng.standard_normal(Corresp.shape)
    R_t = [np.hstack([R, -(R @ C).reshape(3, 1)]) for R, C in cams]
    return np.ascontiguousarray(Corresp), CalM, R_t[1], R_t[2], X


def unit_t2(R_t_2, R_t_3):
    """the ground-truth poses in the scale the estimators return them in: |t2| = 1"""
    s = np.linalg.norm(R_t_2[:, 3])
    a, b = R_t_2.copy(), R_t_3.copy()
    a[:, 3] /= s; b[:, 3] /= s
    return a, b


def calm_item(CalM, b):
    return CalM[b] if np.ndim(CalM) == 3 else CalM


# ---- the comparison the GPU and the emulator tests share -----------------------------------------------------------------------------------------
def has_score_tie(votes8):
    """votes8: the eight cheirality scores of one triplet (debug record [60:68]: four candidates for view 2, four for view 3).  True when two of the
    four scores of either call share the largest value: the reference's winner then depends on the sign convention of svd(E), which MATLAB leaves open."""
    for v in (votes8[0:4], votes8[4:8]):
        v = sorted(float(x) for x in v)
        if v[3] == v[2]:                                                     # the largest score occurs twice: `>=` keeps whichever candidate comes later
            return True
    return False


_ORACLE_CACHE = {}


def oracle_refs(method, C, CalM, key=None):
    """[(oracle outputs, oracle outputs with K2 and K3 exchanged, the oracle's own eight vote scores)] per item; cached under `key` so that the kernel
    routes share one reference"""
    from oracle import tft_oracle as O
    if key is not None and key in _ORACLE_CACHE:
        return _ORACLE_CACHE[key]
    fn = getattr(O, method)
    refs = []
    core = O._recover_R_t_core
    for b in range(C.shape[0]):
        Cb = C[b].T.copy(); Kb = calm_item(CalM, b)
        seen = []

        def spy(E, P1cam, K2, x1, x2, return_debug=False):
            r = core(E, P1cam, K2, x1, x2, True)
            seen.extend(r[2])
            return r if return_debug else r[:2]
        O._recover_R_t_core = spy
        try:
            ref = fn(Cb, Kb)
        finally:
            O._recover_R_t_core = core
        refs.append((ref, fn(Cb, swap_views_23(Kb)), seen[:8]))
    if key is not None:
        _ORACLE_CACHE[key] = refs
    return refs


def check_pose_batch(out, method, C, CalM, tol, refs, votes=None, same_iter=False, what=""):
    """`out`: numpy outputs of a pose_batch-shaped call.  Every item: status 0; T up to sign, R_t_2, R_t_3 and Reconst against the oracle within `tol`,
    directly -- through the 16 sign conventions of svd(E) only for an item whose own vote scores (`votes`, the kernel's debug record) show a tie, at
    most one per call; `iter` equal where asked.  votes=None, for OptimF, which has no debug record in the library: the scores the oracle computes for
    the item (integers, from fundamental matrices that agree with the kernel's to 1e-12) stand in.  Control: the oracle under swap_views_23(CalM) is further than 1e-3 from every item's poses.  Returns (worst error, smallest control distance)."""
    from oracle import tft_oracle as O
    from helpers import rel_err, pose_err, pose_err_any_convention
    B = C.shape[0]
    assert np.all(np.asarray(out["status"]) == 0), (what, np.asarray(out["status"]).tolist())
    worst, control, ties = 0.0, np.inf, 0
    for b in range(B):
        ref, swapped, oracle_votes = refs[b]
        ob = {k: np.asarray(out[k][b]) for k in ("T", "R_t_2", "R_t_3")}
        Cb = C[b].T.copy(); Kb = calm_item(CalM, b)
        e = pose_err(ob, ref)
        rec_ref = ref[2]
        if not e < tol and has_score_tie(votes[b] if votes is not None else oracle_votes):
            ties += 1
            e = pose_err_any_convention(ob, getattr(O, method), Cb, Kb)[1]
            rec_ref = O._final_reconst(Kb, ob["R_t_2"], ob["R_t_3"], Cb)
        if out.get("Reconst") is not None:
            e = max(e, rel_err(np.asarray(out["Reconst"][b]), rec_ref))
        assert e < tol, "%s item %d: %.3e from the oracle (gate %.0e)" % (what, b, e, tol)
        if same_iter:
            assert int(out["iter"][b]) == int(ref[4]), "%s item %d: iter %d, oracle %d" % (what, b, int(out["iter"][b]), int(ref[4]))
        worst = max(worst, e)
        d = max(rel_err(ob["R_t_2"], swapped[0]), rel_err(ob["R_t_3"], swapped[1]))
        assert d > 1e-3, "%s item %d: the oracle with K2 and K3 exchanged is only %.3e away -- the case cannot see a view mix-up" % (what, b, d)
        control = min(control, d)
    assert ties <= 1, "%s: %d items needed the tie rule" % (what, ties)
    return worst, float(control)


# ---- well-posed items --------------------------------------------------------------------------------------------------------------------------------------
def oracle_sensitivity(method, Cb, Kb, ref=None):
    """How far the oracle's own result (T up to sign, R_t_2, R_t_3, Reconst; relative, as the gates measure) moves when every coordinate of its input
    moves by four units in the last place, in a fixed pattern of signs."""
    from oracle import tft_oracle as O
    from helpers import rel_err, rel_err_T
    fn = getattr(O, method)
    if ref is None:
        ref = fn(Cb, Kb)
    sg = np.random.default_rng(0).choice([-1.0, 1.0], size=Cb.shape)
    alt = fn(Cb * (1.0 + 4 * np.finfo(float).eps * sg), Kb)
    return max(rel_err_T(alt[3], ref[3]), rel_err(alt[0], ref[0]), rel_err(alt[1], ref[1]), rel_err(alt[2], ref[2]))


def well_posed_batch(name, B, N, noise, seed, K, method, tol):
    """rig_batch(name, B, N, noise, seed, K) with every item redrawn (item b of the batch of seed + 1000, + 2000, ...) while the ORACLE's result for it
    moves by more than tol / 100 under oracle_sensitivity's change of the input by 4 ulp.  Such an item is ill-posed for a gate of `tol` whatever computes
    it -- a kernel reads the same data and rounds a thousand operations differently -- and minimal samples at 0.5 px noise produce some (eight noisy
    points leave OptimF's Gauss-Helmert iteration one redundant constraint).  The criterion never looks at a kernel's output."""
    C, CalM, R2, R3, X = rig_batch(name, B, N, noise, seed, K)
    for b in range(B):
        j = 0
        while oracle_sensitivity(method, C[b].T.copy(), calm_item(CalM, b)) > tol / 100:
            j += 1
            assert j < 20, "no well-posed item %d for %s N=%d" % (b, name, N)
            Cj, _, _, _, Xj = rig_batch(name, B, N, noise, seed + 1000 * j, K)
            C[b], X[b] = Cj[b], Xj[b]
    return C, CalM, R2, R3, X
