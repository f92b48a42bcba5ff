"""
Robust losses in the three-view bundle adjustment (include/tftfund_loss.h), the part that needs no GPU: the header, the symbol list and the library;
the argument errors of the entry points and of the Python wrappers, raised before a device is touched; and the numpy restatement
(tests/ba_loss_oracle.py) against finite differences, against least squares in the pixel metric, and on the scene the end-to-end GPU test leans on.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import ba_oracle as BA
from tft_vs_fund_amd import api
from tft_vs_fund_amd.build import build_library

import ba_loss_cases as bc
import ba_loss_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tff_bundle_adjust_loss_batch_dev", "tff_bundle_adjust_loss_batch_host", "tff_bundle_adjust_loss_ragged_dev",
               "tff_bundle_adjust_loss_ragged_host"]
CALM = np.tile(np.diag([800.0, 800.0, 1.0]), (3, 1))


class _NoLibrary(api.Context):
    """the wrappers of Context without a context behind them"""

    def __init__(self):
        self.device = 0

    def __del__(self):
        pass


# ---- declarations and argument errors ------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_and_exported():
    main = open(os.path.join(ROOT, "include", "tftfund.h")).read()
    includes = re.findall(r'^#include "(tftfund_\w+\.h)"', main, flags=re.M)
    assert includes[-1] == "tftfund_loss.h" and includes.count("tftfund_loss.h") == 1                 # included last
    txt = open(os.path.join(ROOT, "include", "tftfund_loss.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tff_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(api.LOSS_SYMBOLS) == sorted(NEW_SYMBOLS)
    assert not set(api.LOSS_SYMBOLS) & (set(api.EXPORTED_SYMBOLS) | set(api.ADAPTIVE_SYMBOLS) | set(api.GUIDED_SYMBOLS))
    assert re.findall(r"#define (TFF_LOSS_\w+) (\d+)", txt) == [("TFF_LOSS_NONE", "0"), ("TFF_LOSS_HUBER", "1"), ("TFF_LOSS_CAUCHY", "2")]
    assert api.LOSS_IDS == {"huber": 1, "cauchy": 2}
    build_library()
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.tff_version() >= 106


def test_header_compiles_as_c_in_either_order(tmp_path):
    for n, first in enumerate(("tftfund.h", "tftfund_loss.h")):
        src = tmp_path / ("t%d.c" % n)
        src.write_text('#include "%s"\n#include "tftfund.h"\n#include "tftfund_loss.h"\n'
                       'int (*p)(tff_ctx*, const double*, int64_t, const double*, const double*, const double*, int64_t, int32_t, const double*, double*, double*,\n'
                       '         double*, int32_t*, double*, int32_t*, int32_t, double, double*) = tff_bundle_adjust_loss_batch_dev;\n'
                       'int loss = TFF_LOSS_CAUCHY;\n' % first)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_entry_points_refuse_a_null_context():
    build_library()
    lib = api.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "tff_bundle_adjust_loss_batch_dev": (None, p, 0, p, p, p, 1, 8, None, p, p, p, p, p, p, 1, 3.0, p),
        "tff_bundle_adjust_loss_batch_host": (None, p, 0, p, p, p, 1, 8, None, p, p, p, p, p, p, 2, 3.0, p),
        "tff_bundle_adjust_loss_ragged_dev": (None, p, p, 8, None, p, 0, p, p, None, 1, p, p, p, p, p, p, p, 1, 3.0, p),
        "tff_bundle_adjust_loss_ragged_host": (None, p, p, None, p, 0, p, p, None, 1, p, p, p, p, p, p, p, 0, 0.0, None),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -10001, name
        assert lib.tff_last_error().decode() == "null context", name


def test_python_argument_errors_come_before_the_library():
    ctx = _NoLibrary()
    C = np.zeros((1, 12, 6)); Rt = np.zeros((1, 3, 4))
    packed = np.zeros((20, 6)); off = np.array([0, 10, 20], dtype=np.int64); Rt2 = np.zeros((2, 3, 4))
    bad = [dict(loss="l2", scale=1.0), dict(loss="Huber", scale=1.0), dict(loss=1, scale=1.0),              # the name
           dict(scale=3.0),                                                                                # a scale without a loss
           dict(loss="huber"), dict(loss="huber", scale=0.0), dict(loss="cauchy", scale=-1.0), dict(loss="cauchy", scale=float("nan")),
           dict(loss="cauchy", scale=float("inf")), dict(loss="huber", scale="3"), dict(loss="huber", scale=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.bundle_adjust(CALM, Rt, Rt, C, **kw)
        with pytest.raises(ValueError):
            ctx.bundle_adjust_ragged(CALM, Rt2, Rt2, packed, off, **kw)
    polish_bad = [dict(polish_loss="l2"), dict(polish_scale=2.0), dict(polish_loss="huber", polish_scale=0.0), dict(polish_loss="cauchy", polish_scale=-2.0),
                  dict(polish_all=True), dict(polish_all=True, polish_scale=2.0)]
    for kw in polish_bad:
        for polish in (False, True):                                          # argument errors whether or not the polish runs
            with pytest.raises(ValueError):
                ctx.robust_pose_scenes("LinearTFTPoseEstimation", packed, off, CALM, 100, 4.0, polish=polish, **kw)
            with pytest.raises(ValueError):
                ctx.robust_pose("LinearFPoseEstimation", packed, CALM, 100, 4.0, polish=polish, **kw)
    with pytest.raises(ValueError):                                            # polish_scale defaults to the threshold, which must then do as a scale
        ctx.robust_pose_scenes("LinearTFTPoseEstimation", packed, off, CALM, 100, -1.0, polish_loss="huber")
    # valid arguments go on to the (absent) library
    with pytest.raises(AttributeError):
        ctx.robust_pose_scenes("LinearTFTPoseEstimation", packed, off, CALM, 100, 4.0, polish_loss="cauchy", polish_all=True)
    with pytest.raises(AttributeError):
        ctx.bundle_adjust_ragged(CALM, Rt2, Rt2, packed, off, loss="huber", scale=3)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,c", (("huber", 3.0), ("cauchy", 3.0), ("huber", 150.0), (None, None)))
def test_gradient_against_finite_differences(loss, c):
    """the gradient the reweighted loop descends along, 2 J' diag(rho' / s^2) r, is that of F = sum rho(|e|^2); N = 12, at the start, where the
    residuals (some 150 px) lie on the linear side of Huber at 3 px and on both sides at 150 px"""
    sc = bc.scene(12, 0)
    x, Cn, Kn, s = LO.prepare(sc["CalM"], sc["R_t_0"], sc["C"].T.copy(), sc["X0"].T.copy())
    F0, g = LO.cost_and_gradient(x, Cn, Kn, s, loss, c)
    if loss == "huber":
        e2 = LO.e2_of(BA.bundleadjustment_LM(x, Cn, Kn, False), s)
        assert (e2 > c * c).any() and ((e2 <= c * c).any() or c == 3.0)
    # central differences with h = 1e-6 |x_k|-ish steps: truncation ~ h^2 F''' and rounding ~ eps F / h, both far below 1e-6 of the gradient's size
    h = 1e-6
    for k in list(range(12)) + [12, 25, 47]:
        e = np.zeros(x.size); e[k] = h
        fd = (LO.cost_and_gradient(x + e, Cn, Kn, s, loss, c)[0] - LO.cost_and_gradient(x - e, Cn, Kn, s, loss, c)[0]) / (2 * h)
        assert abs(fd - g[k]) <= 1e-6 * np.abs(g).max(), (k, fd, g[k])


@pytest.mark.parametrize("n,n_bad", ((12, 0), (40, 2)))
def test_least_squares_limit(n, n_bad):
    """c = 1e9: every weight is 1 (Huber exactly, Cauchy to 1e-12) and both losses run the least-squares loop in the pixel metric"""
    ref = bc.restated(n, n_bad, None, None, True)
    rel = lambda a, r: np.abs(a - r).max() / np.abs(r).max()
    for loss in ("huber", "cauchy"):
        r = bc.restated(n, n_bad, loss, 1e9, True)
        assert r["iter"] == ref["iter"] and abs(r["repr_err"] - ref["repr_err"]) <= 1e-9 * ref["repr_err"]
        assert rel(r["R_t"], ref["R_t"]) < 1e-9 and rel(r["Reconst"], ref["Reconst"]) < 1e-9 and np.abs(r["weight"] - 1.0).max() < 1e-9


def test_accuracy_condition_on_the_end_to_end_scene():
    """100 matches, 30 displaced: Cauchy at 3 px leaves less than half the rotation error of plain least squares from the same start (a condition on the
    inputs, asserted on the restatement alone; tests/test_gpu_ba_loss.py meets the restatement on this scene)"""
    sc = bc.scene(*bc.BIG)
    r = bc.restated(*bc.BIG, "cauchy", 3.0, False)
    Ro, _, ito, _ = BA.BundleAdjustment(sc["CalM"], sc["R_t_0"], sc["C"].T.copy(), None)
    for j, truth in enumerate(sc["truth"]):
        robust, plain = bc.rot_err_deg(truth, r["R_t"][3 * j + 3:3 * j + 6]), bc.rot_err_deg(truth, Ro[3 * j + 3:3 * j + 6])
        print("view %d: Cauchy %.3f deg, least squares %.3f deg" % (j + 2, robust, plain))
        assert robust < 0.5 * plain
    assert r["margin"] >= 1e-10 and r["weight"][sc["bad"]].max() < 0.1 < np.median(r["weight"])
