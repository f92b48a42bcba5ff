"""
The cases of the bundle adjustment over tracks (include/tftfund_tracks.h), shared by tests/test_emulated_ba_tracks.py (lane emulator) and
tests/test_gpu_ba_tracks.py, with the restatement's result of each (tests/ba_tracks_oracle.py, computed once per process) and the gates.

Synthetic: scenes.generate_multiview_scene, noise 1 px, M in {2, 3, 4, 6} x N in {12, 64, 65, 130} (one trip of 64 lanes, the lane boundary on both
sides, three trips), poses perturbed by ~0.5 degrees / 1 % and given in a frame whose first camera is NOT [I|0]; every case with and without Reconst0.
Visibility patterns (PATTERNS): full; every point missing from up to M - 2 random views, every view keeping >= 60 % of the points; the last view entirely NaN;
view 1 missing from exactly one point; point 0 and point 64 missing from view 1; a NaN in the y coordinate only and an Inf; three points with one
observation and two with none, the last point among them.  Real: three windows of EPFL tracks (tests/golden/epfl_all.npz), cut to 60 - 72 tracks.
Failing items: no point with two observations (ST_TOO_FEW), a view with a single observation (ST_NONFINITE).

Gates (those of tests/test_bundle_adjustment.py): status and used exact, iter equal to the restatement's, repr_err, R_t and the Reconst columns of the
points taking part within 1e-9 relative, NaN exactly at the dropped columns.
"""
import functools
import os

import numpy as np

import ba_tracks_oracle as TO
from tft_vs_fund_amd.scenes import generate_multiview_scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VIEWS = (2, 3, 4, 6)
SIZES = (12, 64, 65, 130)
PATTERNS = ("full", "random", "view_nan", "one_missing", "p0_p64", "y_nan_inf", "few_obs")
SEED = 3
TOL = 1e-9


def applicable(M, N, pattern):
    """the patterns that say something at this size: with two views a point missing from one is dropped, and a view entirely NaN leaves nothing
    (that is the failing item `too_few`); point 64 exists from N = 65 on"""
    if pattern == "view_nan":
        return M >= 3
    if pattern == "random":
        return M >= 3                                                                    # (M - 2 = 0 views: the full pattern)
    if pattern == "p0_p64":
        return N > 64
    return True


SYNTHETIC = [(M, N, p, x0) for M in VIEWS for N in SIZES for p in PATTERNS if applicable(M, N, p) for x0 in (False, True)]


def _perturbed(R_t, rng):
    R0 = R_t.copy()
    for j in range(1, R_t.shape[0] // 3):
        w = 0.01 * rng.standard_normal(3); th = np.linalg.norm(w); k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R0[3 * j:3 * j + 3, :3] = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx) @ R_t[3 * j:3 * j + 3, :3]
        R0[3 * j:3 * j + 3, 3] = R_t[3 * j:3 * j + 3, 3] * (1 + 0.01 * rng.standard_normal(3))
    return R0


@functools.lru_cache(maxsize=None)
def scene(M, N, seed=SEED):
    """the fully visible problem: CalM, R0 (moved frame), C (2M x N), X0 (3 x N, in the frame of R0)"""
    rng = np.random.default_rng(1000 * M + seed)
    C, CalM, R_t, X = generate_multiview_scene(M, N, noise=1.0, seed=10 * M + seed)
    sc = np.linalg.norm(R_t[3:6, 3]); R_t[:, 3] /= sc; X = X / sc
    R0 = _perturbed(R_t, rng)
    X0 = X * (1 + 0.01 * rng.standard_normal(X.shape))
    a = 0.3
    G = np.eye(4); G[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]; G[:3, 3] = [0.2, -0.1, 0.4]
    R0 = np.vstack([R0[3 * j:3 * j + 3] @ G for j in range(M)])
    X0 = (np.linalg.inv(G) @ np.vstack([X0, np.ones(N)]))[:3]
    return CalM, R0, C, X0


def apply_pattern(C, pattern, seed=SEED):
    M, N = C.shape[0] // 2, C.shape[1]
    C = C.copy()
    if pattern == "full":
        pass
    elif pattern == "random":
        rng = np.random.default_rng(77 * M + N + seed)
        while True:
            miss = np.zeros((M, N), dtype=bool)
            for i in range(N):
                miss[rng.permutation(M)[:rng.integers(0, M - 1)], i] = True              # 0 .. M - 2 views
            if (~miss).sum(axis=1).min() >= 0.6 * N:
                break
        C[np.repeat(miss, 2, axis=0)] = np.nan
    elif pattern == "view_nan":
        C[2 * (M - 1):2 * M] = np.nan
    elif pattern == "one_missing":
        C[2:4, N // 2] = np.nan
    elif pattern == "p0_p64":
        C[2:4, 0] = np.nan; C[2:4, 64] = np.nan
    elif pattern == "y_nan_inf":
        C[3, 3] = np.nan                                                                 # y only: the observation does not exist
        C[2 * (M - 1), 5] = np.inf
    elif pattern == "few_obs":
        for k, i in enumerate((1, 7, N - 1)):                                            # one observation each
            keep = k % M
            for v in range(M):
                if v != keep:
                    C[2 * v:2 * v + 2, i] = np.nan
        C[:, 4] = np.nan; C[:, N - 2] = np.nan                                           # none
    else:
        raise ValueError(pattern)
    return C


def synthetic(M, N, pattern, with_x0):
    CalM, R0, C, X0 = scene(M, N)
    return CalM, R0, apply_pattern(C, pattern), (X0 if with_x0 else None)


# ---- real data: windows of consecutive views, tracks merged from consecutive triplets ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _epfl():
    return dict(np.load(os.path.join(GOLDEN, "epfl_all.npz")))


def window_tracks(dataset, first, M, max_px=1.0):
    """Tracks over the images first .. first + M - 1 (1-based, as the fixture numbers them) of `dataset` ("fountain" | "herzjesu"): the matches of the
    triplets (i, i+1, i+2) of the window, merged where a match of one triplet agrees TO THE BIT with a match of the next in the two views they share;
    tracks whose reprojection under the ground-truth cameras exceeds max_px in any seen coordinate removed (experiments_real.m:93-99 does this per
    triplet).  -> Corresp (2M x T, NaN where not seen), CalM (3M x 3), R_t (3M x 4: the ground truth [R_j | t_j] in the world frame), X (3 x T)."""
    g = _epfl()
    trips, off, corr = g[dataset + "_triplets"], g[dataset + "_offsets"], g[dataset + "_corresp"]
    tracks = []                                                                          # rows of 2M, NaN where not seen
    for k in range(M - 2):
        ids = (first + k, first + k + 1, first + k + 2)
        t = [n for n, r in enumerate(trips) if tuple(int(x) for x in r[:3]) == ids]
        if not t:
            raise ValueError("%s has no triplet %r" % (dataset, ids))
        rows = corr[off[t[0]]:off[t[0] + 1]]
        index = {}
        for n, tr in enumerate(tracks):
            key = tr[2 * k:2 * k + 4]
            if np.isfinite(key).all():
                index.setdefault(key.tobytes(), n)
        for r in rows:
            n = index.get(r[0:4].tobytes()) if k > 0 else None
            if n is not None:
                if np.isnan(tracks[n][2 * k + 4]):
                    tracks[n][2 * k + 4:2 * k + 6] = r[4:6]
            else:
                tr = np.full(2 * M, np.nan); tr[2 * k:2 * k + 6] = r
                tracks.append(tr)
    C = np.array(tracks).T
    Ks = [g[dataset + "_K"][first - 1 + j] for j in range(M)]
    Rts = [np.hstack([g[dataset + "_R"][first - 1 + j], g[dataset + "_t"][first - 1 + j].reshape(3, 1)]) for j in range(M)]
    vis = TO.visibility(C)
    X = np.zeros((3, C.shape[1])); keep = np.ones(C.shape[1], dtype=bool)
    from oracle import tft_oracle as O
    for i in range(C.shape[1]):
        js = np.flatnonzero(vis[:, i])
        Xh = O.triangulation3D([Ks[j] @ Rts[j] for j in js], np.concatenate([C[2 * j:2 * j + 2, i:i + 1] for j in js]))
        X[:, i] = Xh[0:3, 0] / Xh[3, 0]
        for j in js:
            p = Ks[j] @ (Rts[j] @ np.append(X[:, i], 1.0))
            if np.abs(p[0:2] / p[2] - C[2 * j:2 * j + 2, i]).max() > max_px:
                keep[i] = False
    return C[:, keep], np.vstack(Ks), np.vstack(Rts), X[:, keep]


REAL = (("fountain", 5, 4, 66), ("herzjesu", 3, 5, 60), ("fountain", 2, 6, 72))        # dataset, first image, views, tracks kept


@functools.lru_cache(maxsize=None)
def real(dataset, first, M, n_tracks, seed=SEED):
    """a window cut to n_tracks tracks by a fixed seed, ground-truth poses perturbed (no Reconst0: the points are triangulated from the views that see them)"""
    C, CalM, R_t, X = window_tracks(dataset, first, M)
    rng = np.random.default_rng(seed + first + 100 * M)
    sel = np.sort(rng.permutation(C.shape[1])[:n_tracks])
    return CalM, _perturbed(R_t, rng), np.ascontiguousarray(C[:, sel]), None


# ---- failing items ------------------------------------------------------------------------------------------------------------------------------------
def failing(kind, M=3, N=12):
    CalM, R0, C, X0 = scene(M, N)
    C = C.copy()
    if kind == "too_few":                                                                # every point seen in one view only
        for i in range(N):
            for v in range(M):
                if v != i % M:
                    C[2 * v:2 * v + 2, i] = np.nan
        return (CalM, R0, C, None), 0, TO.ST_TOO_FEW
    if kind == "single":                                                                 # view 2 sees point 4 and nothing else
        keep = C[4:6, 4].copy(); C[4:6] = np.nan; C[4:6, 4] = keep
        return (CalM, R0, C, X0), N, TO.ST_NONFINITE
    raise ValueError(kind)


FAILING = ("too_few", "single")


# ---- the restatement, once per case ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(kind, *key):
    case = synthetic(*key) if kind == "syn" else real(*key) if kind == "real" else failing(*key)[0]
    return TO.BundleAdjustmentTracks(*case)


def gate(got, ref, what):
    """got, ref: (R_t 3M x 4, Reconst 3 x N, iter, repr_err, used, status)"""
    Rk, Xk, itk, errk, usedk, stk = got
    Ro, Xo, ito, erro, usedo, sto = ref
    assert (int(stk), int(usedk)) == (sto, usedo), what
    if sto != TO.ST_OK:
        assert np.isnan(Rk).all() and np.isnan(Xk).all() and np.isnan(errk) and int(itk) == 0, what
        return
    assert int(itk) == ito, (what, int(itk), ito)
    assert abs(float(errk) - erro) <= TOL * erro, (what, float(errk), erro)
    dropped = np.isnan(Xo).all(axis=0)
    assert np.array_equal(np.isnan(Xk), np.isnan(Xo)) and int((~dropped).sum()) == usedo, what    # NaN exactly at the dropped columns
    eR = np.abs(Rk - Ro).max() / np.abs(Ro).max()
    eX = np.abs(Xk[:, ~dropped] - Xo[:, ~dropped]).max() / np.abs(Xo[:, ~dropped]).max()
    assert eR < TOL and eX < TOL, (what, eR, eX)
    assert np.array_equal(Rk[0:3], np.eye(3, 4)), what
