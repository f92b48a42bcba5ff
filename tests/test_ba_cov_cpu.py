"""
Covariances of the three-view bundle adjustment (include/tftfund_cov.h), the part that needs no GPU: the numpy restatement (tests/ba_cov_oracle.py)
-- its three routes to the cofactor matrix against one another, and its prediction against the scatter of the adjustment's result over redrawn noise --,
api.euler_cov_to_rotvec against finite differences, and the header, the symbol list, the library and the argument errors raised before a device is
touched.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.ba_oracle import BundleAdjustment, _rot_parts
from tft_vs_fund_amd import api
from tft_vs_fund_amd.build import build_library

import ba_cov_cases as cc
import ba_cov_oracle as CO
import ba_loss_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tff_ba_covariance_batch_dev", "tff_ba_covariance_batch_host", "tff_ba_covariance_ragged_dev", "tff_ba_covariance_ragged_host",
               "tff_bundle_adjust_cov_batch_dev", "tff_bundle_adjust_cov_batch_host", "tff_bundle_adjust_cov_ragged_dev", "tff_bundle_adjust_cov_ragged_host"]
CALM = np.tile(np.diag([800.0, 800.0, 1.0]), (3, 1))


class _NoLibrary(api.Context):
    """the wrappers of Context without a context behind them"""

    def __init__(self):
        self.device = 0

    def __del__(self):
        pass


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_bad", ((12, 0), (129, 0), (65, 13), (64, 8), (40, 2)))
@pytest.mark.parametrize("loss,c", cc.LOSSES)
def test_three_routes_to_the_cofactor_matrix_agree(n, n_bad, loss, c):
    """the bordered inverse (the definition), the projected pseudo-inverse and the Schur form the kernel evaluates, at the restated optimum: within
    1e-10 of the largest entry (measured: 5e-12), camera block and point blocks; and the gauge: Q h = 0"""
    sc = bc.scene(n, n_bad)
    R_t, X = cc.optimum(n, n_bad, loss, c)
    x, J, F, m = CO.system(sc["CalM"], R_t, sc["C"].T.copy(), X, loss, c)
    bordered, projected, schur = CO.routes(x, J)
    for other in (projected, schur):
        for k in ("Qc", "Qx"):
            d = np.abs(other[k] - bordered[k]).max() / np.abs(bordered[k]).max()
            assert d <= 1e-10, (k, d)
    h12 = x[:12].copy(); h12[:6] = 0.0; h12[9:] = 0.0
    assert abs(np.linalg.norm(h12) - 1.0) < 1e-12
    assert np.abs(bordered["Qc"] @ h12).max() <= 1e-10 * np.abs(bordered["Qc"]).max()
    ev = np.linalg.eigvalsh(bordered["Qc"])
    assert abs(ev[0]) <= 1e-10 * ev[-1] and ev[1] > 0.0                        # rank 11, positive semi-definite


def test_predicted_covariance_is_the_scatter_of_the_result():
    """T = 300 draws of 1 px noise around the noiseless matches of one scene of 40, the restated adjustment from the truth on each: the standard
    deviation of each of the twelve returned parameters over the mean predicted one is 1 within 5 / sqrt(2 T) (the standard error of a standard
    deviation estimated from T samples, five times)"""
    T = 300
    ms = cc.mc_scene()
    Cs = cc.mc_draws(T)
    params, covs = [], []
    for C in Cs:
        R_t, X = BundleAdjustment(ms["CalM"], ms["R_t_0"], C.T.copy(), ms["X"].T.copy())[0:2]
        params.append(cc.mc_params(R_t[None, 3:6], R_t[None, 6:9])[0])
        covs.append(CO.covariance(ms["CalM"], R_t, C.T.copy(), X)["cov"])
    ratio = cc.mc_ratio(np.array(params), np.array(covs))
    print("empirical / predicted standard deviation:", np.round(ratio, 3))
    assert np.abs(ratio - 1.0).max() <= 5.0 / np.sqrt(2.0 * T), ratio


def test_euler_cov_to_rotvec_against_finite_differences():
    """omega(d) = log(R(angles + d) R(angles)') by central differences, per camera; the translations pass through"""
    rng = np.random.default_rng(3)

    def rot(a):
        Rx, Ry, Rz = _rot_parts(a)[0:3]
        return Rx @ Ry @ Rz

    def log3(R):
        th = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
        return w if th < 1e-12 else w * th / np.sin(th)

    angles = rng.uniform(-1.2, 1.2, (2, 3))
    T = np.eye(12)
    h = 1e-6                                                                     # truncation h^2, rounding eps / h: both 1e-10 and less
    for j in range(2):
        R0 = rot(angles[j])
        for k in range(3):
            e = np.zeros(3); e[k] = h
            T[3 * j:3 * j + 3, 3 * j + k] = (log3(rot(angles[j] + e) @ R0.T) - log3(rot(angles[j] - e) @ R0.T)) / (2 * h)
    A = rng.standard_normal((12, 12)); cov = A @ A.T
    Rt = [np.hstack([rot(angles[j]), rng.standard_normal((3, 1))]) for j in range(2)]
    got = api.euler_cov_to_rotvec(Rt[0], Rt[1], cov)
    want = T @ cov @ T.T
    assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max()
    assert np.array_equal(got[6:, 6:], cov[6:, 6:])
    both = api.euler_cov_to_rotvec(np.stack([Rt[0], Rt[0]]), np.stack([Rt[1], Rt[1]]), np.stack([cov, 2.0 * cov]))
    assert np.array_equal(both[0], got) and np.allclose(both[1], 2.0 * got, rtol=1e-14, atol=0.0)
    with pytest.raises(ValueError):
        api.euler_cov_to_rotvec(Rt[0], Rt[1], cov[:6, :6])


# ---- declarations and argument errors ------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_and_exported():
    main = open(os.path.join(ROOT, "include", "tftfund.h")).read()
    tail = main[main.rindex("#ifdef __cplusplus"):]
    assert re.findall(r'^#include "(tftfund_\w+\.h)"', main, flags=re.M).count("tftfund_cov.h") == 1 and '#include "tftfund_cov.h"' in tail   # at the end
    txt = open(os.path.join(ROOT, "include", "tftfund_cov.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tff_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(api.COV_SYMBOLS) == sorted(NEW_SYMBOLS)
    assert not set(api.COV_SYMBOLS) & (set(api.EXPORTED_SYMBOLS) | set(api.ADAPTIVE_SYMBOLS) | set(api.GUIDED_SYMBOLS) | set(api.LOSS_SYMBOLS))
    build_library()
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.tff_version() >= 107


def test_header_compiles_as_c_in_either_order(tmp_path):
    for n, first in enumerate(("tftfund.h", "tftfund_cov.h")):
        src = tmp_path / ("t%d.c" % n)
        src.write_text('#include "%s"\n#include "tftfund.h"\n#include "tftfund_cov.h"\n'
                       'int (*p)(tff_ctx*, const double*, int64_t, const double*, const double*, const double*, int64_t, int32_t, const double*, int32_t, double,\n'
                       '         double*, double*, double*) = tff_ba_covariance_batch_dev;\n'
                       'int loss = TFF_LOSS_CAUCHY;\n' % first)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_entry_points_refuse_a_null_context():
    build_library()
    lib = api.load_library()
    buf = (ctypes.c_double * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "tff_ba_covariance_batch_dev": (None, p, 0, p, p, p, 1, 8, p, 1, 3.0, p, p, p),
        "tff_ba_covariance_batch_host": (None, p, 0, p, p, p, 1, 8, p, 0, 0.0, p, p, None),
        "tff_ba_covariance_ragged_dev": (None, p, p, 8, None, p, 0, p, p, p, 1, 2, 3.0, p, p, p),
        "tff_ba_covariance_ragged_host": (None, p, p, None, p, 0, p, p, p, 1, 0, 0.0, p, p, None),
        "tff_bundle_adjust_cov_batch_dev": (None, p, 0, p, p, p, 1, 8, None, p, p, p, p, p, p, 1, 3.0, p, p, p, p),
        "tff_bundle_adjust_cov_batch_host": (None, p, 0, p, p, p, 1, 8, None, p, p, p, p, p, p, 2, 3.0, p, p, p, None),
        "tff_bundle_adjust_cov_ragged_dev": (None, p, p, 8, None, p, 0, p, p, None, 1, p, p, p, p, p, p, p, 1, 3.0, p, p, p, p),
        "tff_bundle_adjust_cov_ragged_host": (None, p, p, None, p, 0, p, p, None, 1, p, p, p, p, p, p, p, 0, 0.0, None, p, p, None),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -10001, name                       # TFF_E_INVALID
        assert lib.tff_last_error().decode() == "null context", name


def test_python_argument_errors_come_before_the_library():
    ctx = _NoLibrary()
    packed = np.zeros((20, 6)); off = np.array([0, 10, 20], dtype=np.int64); Rt2 = np.zeros((2, 3, 4))
    for kw in (dict(polish_cov=True), dict(polish_cov=True, polish_loss="huber")):     # the covariance of a polish that does not run
        with pytest.raises(ValueError):
            ctx.robust_pose_scenes("LinearTFTPoseEstimation", packed, off, CALM, 100, 4.0, **kw)
        with pytest.raises(ValueError):
            ctx.robust_pose("LinearFPoseEstimation", packed, CALM, 100, 4.0, **kw)
    with pytest.raises(ValueError):
        ctx.ba_covariance_ragged(CALM, Rt2, Rt2, packed, off, None)
    with pytest.raises(ValueError):
        ctx.ba_covariance_ragged(CALM, Rt2, Rt2, packed, off, np.zeros((19, 3)))
    with pytest.raises(ValueError):
        ctx.ba_covariance_ragged(CALM, Rt2, Rt2, packed, off, np.zeros((20, 3)), loss="huber")
    # valid arguments go on to the (absent) library
    with pytest.raises(AttributeError):
        ctx.ba_covariance_ragged(CALM, Rt2, Rt2, packed, off, np.zeros((20, 3)), loss="huber", scale=3.0, point_cov=True)
    with pytest.raises(AttributeError):
        ctx.bundle_adjust_ragged(CALM, Rt2, Rt2, packed, off, cov=True)
    with pytest.raises(AttributeError):
        ctx.robust_pose_scenes("LinearTFTPoseEstimation", packed, off, CALM, 100, 4.0, polish=True, polish_cov=True)
