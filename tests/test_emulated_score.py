"""
The MSAC score (TFF_OPT_SCORE = 1) of the four count kernels on the lane emulator, no GPU: k_repr_error (with and without the RMS error),
k_inlier_count_staged, k_inlier_count_rows and k_inlier_count_scenes (staged in LDS and read in place, a slab that cuts a scene) compiled by g++
(tests/emu/emu_score.cpp) in their count and MSAC forms.  Scenes of 16, 17, 65 and 130 matches at 0.5 px noise, a quarter of them displaced by 20 - 80 px
in views 2 and 3; nine hypotheses per scene (two full wavefronts of the rows kernel and a tail row): the ground-truth pose and small perturbations of it.

Required: the four MSAC forms give the same integers; the count forms give what k_repr_error gives today; and against numpy -- the emulated
k_triangulate points, then cameras, residuals, rule and weights in double -- the counts are equal and, with F = sum over the numpy inliers of
1 + 63 (1 - ss c), F - count - 1 <= score <= F + 1: the truncation to an integer loses less than one unit per inlier, the +-1 covers a weight whose
real value lies within rounding of an integer.
"""
import ctypes
import os
import subprocess

import numpy as np

from tft_vs_fund_amd import api
from tft_vs_fund_amd.scenes import generate_scene_batch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i, c_d = ctypes.c_long, ctypes.c_int, ctypes.c_double
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None

SIZES = [16, 17, 65, 130]
S = len(SIZES)
B = 9
THR = 4.0
C = 1.0 / (6.0 * THR * THR)


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_score.so")
    deps = [os.path.join(emu, f) for f in ("emu_score.cpp", "emu_primitives.h", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_score.cpp")], check=True)
    return ctypes.CDLL(out)


def _cm(Rt):
    return np.ascontiguousarray(Rt.T).reshape(12)


def _scene(n, seed):
    """(scene (n, 6) with n // 4 matches displaced, CalM (9, 3), Rt2 / Rt3 (B, 12) column-major: hypothesis 0 the truth, the others perturbed)"""
    Cs, CalM, Rt0, _ = generate_scene_batch(1, n, noise=0.5, seed=seed)
    scene = np.ascontiguousarray(Cs[0]).copy()
    rng = np.random.default_rng(100 + seed)
    bad = rng.choice(n, n // 4, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    Rt2 = np.zeros((B, 12)); Rt3 = np.zeros((B, 12))
    for b in range(B):
        e = rng.normal(0, (0.0, 2e-4, 5e-4, 1e-3)[b % 4], (2, 3, 4))
        Rt2[b] = _cm(Rt0[0] + e[0]); Rt3[b] = _cm(Rt0[1] + e[1])
    return scene, np.ascontiguousarray(CalM), Rt2, Rt3


ITEMS = [_scene(n, 11 + k) for k, n in enumerate(SIZES)]


def _one(L, fn, item, msac, err=None):
    scene, CalM, Rt2, Rt3 = item
    counts = np.full(B, -9, dtype=np.int32)
    calm = np.ascontiguousarray(CalM.T).reshape(27)
    args = [P(scene), c_i(scene.shape[0]), P(calm), P(Rt2), P(Rt3), c_l(B), c_d(THR), c_d(C if msac else 0.0), P(counts)]
    if fn == "s_repr":
        args.append(P(err))
    getattr(L, fn)(*args, c_i(msac))
    return counts


def _numpy(L, item):
    """(count, F) per hypothesis from the emulated k_triangulate points: the rule and the untruncated weights in double"""
    scene, CalM, Rt2, Rt3 = item
    n = scene.shape[0]
    cams = np.zeros((B, 3, 3, 4))
    for b in range(B):
        cams[b, 0] = CalM[0:3] @ np.eye(3, 4)
        cams[b, 1] = CalM[3:6] @ Rt2[b].reshape(4, 3).T
        cams[b, 2] = CalM[6:9] @ Rt3[b].reshape(4, 3).T
    cams_cm = np.ascontiguousarray(cams.transpose(0, 1, 3, 2))                  # 3 x 4 column-major each
    X = np.zeros((B, n, 4))
    L.s_triangulate(P(cams_cm), P(scene), c_l(B), c_i(n), P(X))
    cnt = np.zeros(B, dtype=np.int64); F = np.zeros(B)
    for b in range(B):
        ss = np.zeros(n); inl = np.ones(n, dtype=bool)
        for v in range(3):
            proj = X[b] @ cams[b, v].T
            dx = proj[:, 0] / proj[:, 2] - scene[:, 2 * v]; dy = proj[:, 1] / proj[:, 2] - scene[:, 2 * v + 1]
            inl &= (np.abs(dx) <= THR) & (np.abs(dy) <= THR)
            ss += dx * dx + dy * dy
        cnt[b] = inl.sum()
        F[b] = (1.0 + 63.0 * (1.0 - ss[inl] * C)).sum()
    return cnt, F


def test_msac_forms_agree_and_count_forms_are_unchanged():
    L = _lib()
    for item in ITEMS:
        hard = _one(L, "s_repr", item, 0)
        err0 = np.zeros(B); err1 = np.zeros(B)
        assert np.array_equal(_one(L, "s_repr", item, 0, err0), hard)
        for fn in ("s_staged", "s_rows"):
            assert np.array_equal(_one(L, fn, item, 0), hard), fn
        soft = _one(L, "s_repr", item, 1)
        assert np.array_equal(_one(L, "s_repr", item, 1, err1), soft)            # the score does not depend on whether the error is asked for ...
        assert np.array_equal(err0, err1) and (err1 > 0).all()                    # ... nor the error on the score
        for fn in ("s_staged", "s_rows"):
            assert np.array_equal(_one(L, fn, item, 1), soft), fn
        assert (hard <= soft).all() and (soft <= api.SCORE_UNITS * hard.astype(np.int64)).all()
        assert hard[0] > 0                                                        # (hypothesis 0 is the true pose: the comparison is not one of zeros)


def test_scenes_kernel_gives_the_one_scene_integers():
    """36 hypotheses, nine per scene, in slabs of 16: the second slab starts inside scene 1.  stage = 6 * 130: every scene fits (a segment shorter than
    eight hypotheses still reads its scene in place); stage = 6 * 17: the two large scenes are read in place; stage = 0: all are."""
    L = _lib()
    packed, off = api.pack_ragged([it[0] for it in ITEMS])
    calms = np.ascontiguousarray(np.stack([it[1].T.reshape(27) for it in ITEMS]))
    Rt2 = np.ascontiguousarray(np.concatenate([it[2] for it in ITEMS])); Rt3 = np.ascontiguousarray(np.concatenate([it[3] for it in ITEMS]))
    for msac in (0, 1):
        ref = np.concatenate([_one(L, "s_repr", it, msac) for it in ITEMS])
        for stage in (6 * 130, 6 * 17, 0):
            counts = np.full(S * B, -9, dtype=np.int32)
            L.s_scenes(P(packed), P(off), c_l(S), c_l(packed.shape[0]), c_i(130), P(calms), P(Rt2), P(Rt3), c_l(S * B), c_l(B), c_l(16), c_d(THR),
                       c_d(C if msac else 0.0), P(counts), c_i(stage), c_i(msac))
            assert np.array_equal(counts, ref), (msac, stage)


def test_scores_against_numpy():
    L = _lib()
    for item in ITEMS:
        cnt, F = _numpy(L, item)
        hard = _one(L, "s_repr", item, 0); soft = _one(L, "s_repr", item, 1)
        print("N = %d: counts %s scores %s F %s" % (item[0].shape[0], hard.tolist(), soft.tolist(), np.round(F, 2).tolist()))
        assert np.array_equal(hard, cnt)
        assert (F - cnt - 1 <= soft).all() and (soft <= F + 1).all()
