"""
Covariances of the bundle adjustment over tracks (include/tftfund_tracks_cov.h), the part that needs no GPU: the numpy restatement
(tests/ba_tracks_cov_oracle.py) -- its two routes to the cofactor matrix against one another over every case, the three-view restatement
(tests/ba_cov_oracle.py) on fully visible three-view input, the degrees of freedom, the items without a covariance, and its prediction against the
scatter of the adjustment's result over redrawn noise --, api.euler_cov_to_rotvec_views, and the header, the symbol list, the library and the argument
errors raised before a device is touched.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tft_vs_fund_amd import api
from tft_vs_fund_amd.build import build_library

import ba_cov_oracle as CO
import ba_tracks_cases as tc
import ba_tracks_cov_cases as tcc
import ba_tracks_cov_oracle as TCO
import ba_tracks_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tff_ba_tracks_covariance_batch_dev", "tff_ba_tracks_covariance_batch_host", "tff_bundle_adjust_tracks_cov_batch_dev",
               "tff_bundle_adjust_tracks_cov_batch_host"]


class _NoLibrary(api.Context):
    """the wrappers of Context without a context behind them"""

    def __init__(self):
        self.device = 0

    def __del__(self):
        pass


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------------
def test_the_two_routes_agree_and_the_left_out_list_is_what_the_restatement_gives():
    """the dense bordered inverse (the definition) and the Schur form the kernel evaluates, at the restated optimum of every case: within 1e-10 of the
    largest entry of the block, camera block and point blocks, except on the cases of LEFT_OUT -- at most 10 % of the cases and no `full` one"""
    diffs = tcc.check_left_out()
    worst = max(diffs, key=diffs.get)
    print("the two numpy routes: largest difference %.3g at %r; largest among the compared cases %.3g" %
          (diffs[worst], worst, max(d for k, d in diffs.items() if k not in tcc.LEFT_OUT)))
    assert len(tcc.LEFT_OUT) <= len(tcc.CASES) // 10 and not [k for k in tcc.LEFT_OUT if k[2] == "full"]
    for k in tcc.CASES:
        ref = tcc.reference(*k)
        est = ref["est"]
        Qc = ref["cov"]
        assert np.isfinite(Qc).all() and np.allclose(Qc, Qc.T, rtol=0, atol=1e-12 * np.abs(Qc).max()), k
        assert np.abs(Qc @ ref["hP"]).max() <= 1e-9 * np.linalg.norm(Qc, 2), k            # the gauge: cov h_P = 0
        assert not Qc[~est].any() and not Qc[:, ~est].any(), k                            # an unseen camera is a constant
        assert (k[2] == "view_nan") == (not est.all()), k
        ev = np.linalg.eigvalsh(Qc[np.ix_(est, est)])
        assert abs(ev[0]) <= 1e-9 * ev[-1] and ev[1] > 0.0, k                             # rank 6 C_s - 1, positive semi-definite
        CalM, _, C, _ = tcc.inputs(*k[0:4])
        vis = TO.visibility(C); take = vis.sum(axis=0) >= 2
        assert np.array_equal(np.isnan(ref["point_cov"]).all(axis=1), ~take) and not np.isnan(ref["point_cov"][take]).any(), k
        assert ref["dof"] == 2 * int(vis[:, take].sum()) - (int(est.sum()) + 3 * int(take.sum()) - 1), k


def test_degrees_of_freedom():
    assert TCO.dof_of(3 * 40, 2, 40) == 3 * 40 - 11                                     # three fully visible views: as include/tftfund_cov.h
    assert TCO.dof_of(2 * 5, 1, 5) == 0 and TCO.dof_of(2 * 6, 1, 6) == 1                 # two views: five points determine the pose
    assert TCO.dof_of(6 * 10 - 7, 5, 10) == 2 * 53 - (30 + 30 - 1)


@pytest.mark.parametrize("N", (12, 65))
def test_fully_visible_three_views_equal_the_three_view_restatement(N):
    """camera 1 = [I|0], no loss: tests/ba_cov_oracle.py, to 1e-9 of the largest entry"""
    CalM, _, C, _ = tcc.inputs(3, N, "full", None)
    R_t, X = tcc.optimum(3, N, "full", None, None)
    assert np.array_equal(R_t[0:3], np.eye(3, 4))
    a = tcc.reference(3, N, "full", None, None)
    b = CO.covariance(CalM, R_t, C, X)
    assert a["dof"] == 3 * N - 11
    assert np.abs(a["cov"] - b["cov"]).max() <= 1e-9 * np.abs(b["cov"]).max()
    assert abs(a["sigma0"] - b["sigma0"]) <= 1e-9 * b["sigma0"]
    assert (np.abs(a["point_cov"] - b["point_cov"]).max(axis=1) <= 1e-9 * np.abs(b["point_cov"]).max(axis=1)).all()


@pytest.mark.parametrize("kind", tcc.FAILING)
def test_items_without_a_covariance(kind):
    M, CalM, R_t, C, X = tcc.failing(kind)
    for loss, c in tcc.LOSSES:
        ref = TCO.covariance(CalM, R_t, C, X, loss, c)
        assert ref["cov"].shape == (6 * (M - 1),) * 2 and np.isnan(ref["cov"]).all() and np.isnan(ref["sigma0"]) and np.isnan(ref["point_cov"]).all()


def test_predicted_covariance_is_the_scatter_of_the_result():
    """the scene of the GPU test (M = 4, N = 64, the `random` pattern), T = 300 draws of its 2 048 with the restated adjustment from the truth on each:
    the standard deviation of each of the 18 returned parameters over the mean predicted one is 1 within 5 / sqrt(2 (T - 1))"""
    T = 300
    ms = tcc.mc_scene()
    Cs = tcc.mc_draws()[:T]
    poses, covs = [], []
    for C in Cs:
        R_t, X = TO.BundleAdjustmentTracks(ms["CalM"], ms["R_t"], C.T.copy(), ms["X"].copy())[0:2]
        poses.append(R_t)
        covs.append(TCO.covariance(ms["CalM"], R_t, C.T.copy(), X)["cov"])
    ratio = tcc.mc_ratio(tcc.mc_params(np.array(poses)), np.array(covs))
    print("empirical / predicted standard deviation:", np.round(ratio, 3))
    assert np.abs(ratio - 1.0).max() <= 5.0 / np.sqrt(2.0 * (T - 1)), ratio


def test_euler_cov_to_rotvec_views_is_the_three_view_map_per_camera():
    rng = np.random.default_rng(5)
    R_t, _ = tcc.optimum(3, 12, "full", None, None)
    A = rng.standard_normal((12, 12)); cov = A @ A.T
    assert np.array_equal(api.euler_cov_to_rotvec_views(R_t, cov), api.euler_cov_to_rotvec(R_t[3:6], R_t[6:9], cov))
    R6, _ = tcc.optimum(6, 12, "full", None, None)
    A = rng.standard_normal((30, 30)); cov6 = A @ A.T
    got = api.euler_cov_to_rotvec_views(np.stack([R6, R6]), np.stack([cov6, 2.0 * cov6]))
    assert got.shape == (2, 30, 30) and np.array_equal(got[0][15:, 15:], cov6[15:, 15:]) and np.allclose(got[1], 2.0 * got[0], rtol=1e-14, atol=0.0)
    sel = [9, 10, 11, 12, 13, 14, 24, 25, 26, 27, 28, 29]                                # cameras 5 and 6 alone: the three-view map on their block
    assert np.allclose(got[0][np.ix_(sel, sel)], api.euler_cov_to_rotvec(R6[12:15], R6[15:18], cov6[np.ix_(sel, sel)]), rtol=1e-13, atol=0.0)
    for bad in ((R6, cov6[:12, :12]), (R6[:17], cov6), (np.zeros((21, 4)), np.zeros((36, 36)))):
        with pytest.raises(ValueError):
            api.euler_cov_to_rotvec_views(*bad)


# ---- declarations and argument errors ------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_and_exported():
    main = open(os.path.join(ROOT, "include", "tftfund.h")).read()
    tail = main[main.rindex("#ifdef __cplusplus"):]
    assert re.findall(r'^#include "(tftfund_\w+\.h)"', main, flags=re.M).count("tftfund_tracks_cov.h") == 1 and '#include "tftfund_tracks_cov.h"' in tail
    txt = open(os.path.join(ROOT, "include", "tftfund_tracks_cov.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tff_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(api.TRACKS_COV_SYMBOLS) == sorted(NEW_SYMBOLS)
    older = set(api.EXPORTED_SYMBOLS) | set(api.ADAPTIVE_SYMBOLS) | set(api.GUIDED_SYMBOLS) | set(api.LOSS_SYMBOLS) | set(api.COV_SYMBOLS) | set(api.TRACKS_SYMBOLS) \
        | set(api.TRACKS_LOSS_SYMBOLS)
    assert not set(api.TRACKS_COV_SYMBOLS) & older
    # the combined call's argument list is that of the tracks-loss call followed by cov, sigma0, point_cov
    loss_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tftfund_tracks_loss.h")).read(), flags=re.S)
    norm = lambda a: [" ".join(x.split()) for x in a.split(",")]
    for suffix in ("dev", "host"):
        theirs = re.search(r"int tff_bundle_adjust_tracks_loss_batch_%s\((.*?)\);" % suffix, loss_h, flags=re.S).group(1)
        mine = re.search(r"int tff_bundle_adjust_tracks_cov_batch_%s\((.*?)\);" % suffix, code, flags=re.S).group(1)
        assert norm(mine) == norm(theirs) + ["double* cov", "double* sigma0", "double* point_cov"]
    build_library()
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.tff_version() >= 110


def test_header_compiles_as_c_in_either_order(tmp_path):
    for n, first in enumerate(("tftfund.h", "tftfund_tracks_cov.h")):
        src = tmp_path / ("t%d.c" % n)
        src.write_text('#include "%s"\n#include "tftfund.h"\n#include "tftfund_tracks_cov.h"\n'
                       'int (*p)(tff_ctx*, int32_t, const double*, int64_t, const double*, const double*, int64_t, int32_t, const double*, int32_t, double,\n'
                       '         double*, double*, double*) = tff_ba_tracks_covariance_batch_host;\n'
                       'int loss = TFF_LOSS_CAUCHY;\n' % first)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_entry_points_refuse_a_null_context():
    build_library()
    lib = api.load_library()
    buf = (ctypes.c_double * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "tff_ba_tracks_covariance_batch_dev": (None, 3, p, 0, p, p, 1, 8, p, 1, 3.0, p, p, p),
        "tff_ba_tracks_covariance_batch_host": (None, 3, p, 0, p, p, 1, 8, p, 0, 0.0, p, p, None),
        "tff_bundle_adjust_tracks_cov_batch_dev": (None, 3, p, 0, p, p, 1, 8, None, p, p, p, p, p, p, 1, 1.5, p, p, p, p),
        "tff_bundle_adjust_tracks_cov_batch_host": (None, 3, p, 0, p, p, 1, 8, None, p, p, p, p, p, p, 2, 3.0, p, p, p, None),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -10001, name                       # TFF_E_INVALID
        assert lib.tff_last_error().decode() == "null context", name


def test_python_argument_errors_come_before_the_library():
    ctx = _NoLibrary()
    M, B, N = 3, 2, 10
    calm = np.tile(np.diag([800.0, 800.0, 1.0]), (M, 1)); rt = np.zeros((B, 3 * M, 4)); C = np.zeros((B, N, 2 * M)); X = np.zeros((B, 3, N))
    for kw in (dict(cov=True), dict(point_cov=True), dict(missing="view", cov=True), dict(missing="view", cov=True, point_cov=True)):
        with pytest.raises(ValueError):                                      # a covariance needs missing="point"
            ctx.bundle_adjust_views(calm, rt, C, None, **kw)
    with pytest.raises(ValueError):                                          # the loss is still judged
        ctx.bundle_adjust_views(calm, rt, C, None, missing="point", loss="huber", cov=True)
    with pytest.raises(ValueError):                                          # ... and the shapes
        ctx.bundle_adjust_views(calm, rt, np.zeros((B, N, 5)), None, missing="point", cov=True)
    bad = [dict(reconst=None), dict(reconst=np.zeros((B, 3, N + 1))), dict(loss="tukey", scale=1.0), dict(loss="huber"), dict(loss="cauchy", scale=-3.0),
           dict(scale=3.0, loss=1), dict(corresp=np.zeros((B, N, 5))), dict(corresp=np.zeros((B, N, 14))), dict(R_t=np.zeros((B, 3 * M + 3, 4))),
           dict(calm=np.zeros((3 * M + 3, 3)))]
    for kw in bad:
        a = dict(calm=calm, R_t=rt, corresp=C, reconst=X); a.update(kw)
        with pytest.raises(ValueError):
            ctx.ba_tracks_covariance(**a)
    # valid arguments go on to the (absent) device or library
    with pytest.raises((AttributeError, RuntimeError)):
        ctx.ba_tracks_covariance(calm, rt, C, X, loss="huber", scale=3.0, point_cov=True)
    with pytest.raises((AttributeError, RuntimeError)):
        ctx.bundle_adjust_views(calm, rt, C, None, missing="point", cov=True, point_cov=True)
