"""
The bundle adjustment over tracks with a robust loss (include/tftfund_tracks_loss.h), the part that needs no GPU.  The restatement
(tests/ba_tracks_loss_oracle.py): its gradient against central differences, its agreement with the three-view loss restatement where both are least
squares in pixels, its reproducibility under a permuted elimination order, every system it solves Cholesky-positive, and the cap on the cases left out of
the kernel comparisons.  The interface: the header, the symbol list and the library agree, the header compiles as C in either order, the entry points
refuse a null context, and the Python wrappers refuse a bad loss= / scale= before a device is touched.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ba_loss_cases as bl
import ba_loss_oracle as LO
import ba_tracks_loss_cases as lc
import ba_tracks_loss_oracle as TLO
from tft_vs_fund_amd import api
from tft_vs_fund_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tff_bundle_adjust_tracks_loss_batch_dev", "tff_bundle_adjust_tracks_loss_batch_host"]


@pytest.mark.parametrize("loss,c", lc.LOSSES + (("huber", 40.0),))
def test_gradient_against_central_differences(loss, c):
    """F = sum rho(|e_{v,i}|^2) per observation and 2 J' diag(rho' / s^2) r on a partially visible case with displaced observations (at c = 40 px some of
    them are on Huber's quadratic part and some on its linear part)"""
    CalM, R0, C, X0, _ = lc.inputs(4, 12, "random")
    p = TLO.prepare(CalM, R0, C, X0)
    assert p["status"] == 0 and not p["vis"].all()
    x = p["x0"]
    F0, g = TLO.cost_and_gradient(x, p["Corresp_n"], p["CalM_n"], p["s"], loss, c)
    e2 = TLO.e2_of(TLO.bundleadjustment_LM(x, p["Corresp_n"], p["CalM_n"], False), p["s"])[p["vis"].T]
    assert (e2 > c * c).any() and (e2 < c * c).any()
    worst = 0.0
    for k in np.random.default_rng(2).permutation(x.size)[:16]:
        h = 1e-6 * max(1.0, abs(x[k]))
        e = np.zeros(x.size); e[k] = h
        num = (TLO.cost_and_gradient(x + e, p["Corresp_n"], p["CalM_n"], p["s"], loss, c)[0] - TLO.cost_and_gradient(x - e, p["Corresp_n"], p["CalM_n"], p["s"], loss, c)[0]) / (2 * h)
        worst = max(worst, abs(num - g[k]) / max(1.0, abs(g[k])))
    assert worst < 1e-5, worst                                               # (central differences of a function of size 1e4 .. 1e6: 1e-16 F / h)


@pytest.mark.parametrize("n,n_bad", [(12, 0), (64, 8), (65, 13), (129, 0)])
@pytest.mark.parametrize("with_x0", [False, True])
def test_agrees_with_the_three_view_loss_restatement_where_both_are_least_squares(n, n_bad, with_x0):
    """fully visible, camera 1 = [I|0], Huber at c = 1e6 px: per observation or per correspondence, every weight is 1"""
    sc = bl.scene(n, n_bad)
    X0 = sc["X0"].T.copy() if with_x0 else None
    a = TLO.ba_tracks_loss(sc["CalM"], sc["R_t_0"], sc["C"].T.copy(), X0, "huber", 1e6)
    b = LO.ba_loss(sc["CalM"], sc["R_t_0"], sc["C"].T.copy(), X0, "huber", 1e6)
    assert a["status"] == 0 and a["used"] == n and a["iter"] == b["iter"], (a["iter"], b["iter"])
    assert np.abs(a["R_t"] - b["R_t"]).max() < 1e-9 and (a["weight"] == 1.0).all()
    assert abs(a["repr_err"] - b["repr_err"]) <= 1e-9 * b["repr_err"]


@pytest.mark.parametrize("M,N,pattern,loss,c", [(2, 65, "few_obs", "huber", 1.5), (3, 64, "random", "cauchy", 3.0), (4, 65, "view_nan", "huber", 1.5),
                                                (6, 12, "random", "cauchy", 3.0), (6, 64, "few_obs", "huber", 1.5), (4, 130, "full", "cauchy", 3.0)])
def test_reproducible_under_a_permuted_elimination_order(M, N, pattern, loss, c):
    CalM, R0, C, X0, _ = lc.inputs(M, N, pattern)
    a = lc.restated(M, N, pattern, loss, c)
    perm = np.random.default_rng(11).permutation(a["x"].size)
    b = TLO.ba_tracks_loss(CalM, R0, C, X0, loss, c, perm=perm)
    m = ~np.isnan(a["weight"])
    assert a["iter"] == b["iter"] and np.abs(a["R_t"] - b["R_t"]).max() < 1e-11 and np.abs(a["weight"][m] - b["weight"][m]).max() < 1e-11


def test_every_system_is_cholesky_positive_and_few_cases_are_left_out():
    for k in lc.CASES:
        r = lc.restated(*k)
        assert r["status"] == 0 and len(r["chol"]) >= r["iter"] >= 1 and all(r["chol"]), k
        assert r["margin"] >= lc.MIN_MARGIN, (k, r["margins"])               # (none is left out for a tie)
    out = lc.check_left_out()
    assert all(k[3:] == ("huber", 1.5) for k in out)


def test_the_unseen_camera_and_the_dropped_points_of_the_restatement():
    CalM, R0, C, X0, _ = lc.inputs(4, 65, "view_nan")
    r = lc.restated(4, 65, "view_nan", "cauchy", 3.0)
    p = r["prep"]
    assert not p["seen"][3] and p["s"][3] == 1.0 and np.isnan(r["weight"][:, 3]).all()
    assert np.array_equal(r["x"][6:9], p["x0"][6:9]) and np.array_equal(r["x"][15:18], p["x0"][15:18])       # it keeps its start exactly
    r = lc.restated(6, 64, "few_obs", "huber", 1.5)
    dropped = ~r["prep"]["take"]
    assert dropped.sum() == 5 and np.isnan(r["weight"][dropped]).all() and np.isnan(r["Reconst"][:, dropped]).all()
    vis = lc.TO.visibility(lc.inputs(6, 64, "few_obs")[2])
    assert np.array_equal(~np.isnan(r["weight"]), (vis & ~dropped[None]).T)


# ---- the interface ---------------------------------------------------------------------------------------------------------------------------------------
class _NoLibrary(api.Context):
    """the wrappers of Context without a context behind them"""

    def __init__(self):
        self.device = 0

    def __del__(self):
        pass


def test_entry_points_declared_listed_and_exported():
    main = open(os.path.join(ROOT, "include", "tftfund.h")).read()
    tail = main[main.rindex("#ifdef __cplusplus"):]
    assert re.findall(r'^#include "(tftfund_\w+\.h)"', main, flags=re.M).count("tftfund_tracks_loss.h") == 1 and '#include "tftfund_tracks_loss.h"' in tail
    txt = open(os.path.join(ROOT, "include", "tftfund_tracks_loss.h")).read()
    assert "8 B N M bytes" in txt and "per OBSERVATION".lower() in txt.lower()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tff_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(api.TRACKS_LOSS_SYMBOLS) == sorted(NEW_SYMBOLS)
    older = set(api.EXPORTED_SYMBOLS) | set(api.ADAPTIVE_SYMBOLS) | set(api.GUIDED_SYMBOLS) | set(api.LOSS_SYMBOLS) | set(api.COV_SYMBOLS) | set(api.TRACKS_SYMBOLS)
    assert not set(api.TRACKS_LOSS_SYMBOLS) & older
    # the argument list is that of the plain tracks call followed by loss, scale, weight
    plain = re.search(r"int tff_bundle_adjust_tracks_batch_dev\((.*?)\);", open(os.path.join(ROOT, "include", "tftfund_tracks.h")).read(), flags=re.S).group(1)
    norm = lambda a: [" ".join(x.split()) for x in a.split(",")]
    for name in NEW_SYMBOLS:
        mine = re.search(r"int %s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert norm(mine) == norm(plain) + ["int32_t loss", "double scale", "double* weight"]
    build_library()
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.tff_version() >= 109


def test_header_compiles_as_c_in_either_order(tmp_path):
    for n, first in enumerate(("tftfund.h", "tftfund_tracks_loss.h")):
        src = tmp_path / ("t%d.c" % n)
        src.write_text('#include "%s"\n#include "tftfund.h"\n#include "tftfund_tracks_loss.h"\n'
                       'int (*p)(tff_ctx*, int32_t, const double*, int64_t, const double*, const double*, int64_t, int32_t, const double*, double*, double*,\n'
                       '         int32_t*, double*, int32_t*, int32_t*, int32_t, double, double*) = tff_bundle_adjust_tracks_loss_batch_host;\n'
                       'int loss = TFF_LOSS_CAUCHY;\n' % first)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_entry_points_refuse_a_null_context():
    build_library()
    lib = api.load_library()
    buf = (ctypes.c_double * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in NEW_SYMBOLS:
        assert getattr(lib, name)(None, 3, p, 0, p, p, 1, 8, None, p, p, p, p, p, p, 1, 1.5, p) == -10001, name      # TFF_E_INVALID
        assert lib.tff_last_error().decode() == "null context", name


def test_python_argument_errors_come_before_the_library():
    ctx = _NoLibrary()
    M, B, N = 3, 2, 10
    calm = np.tile(np.diag([800.0, 800.0, 1.0]), (M, 1)); rt = np.zeros((B, 3 * M, 4)); C = np.zeros((B, N, 2 * M))
    bad = [dict(missing="point", loss="tukey", scale=1.0), dict(missing="point", loss=1, scale=1.0), dict(missing="point", loss="huber"),
           dict(missing="point", loss="huber", scale=0.0), dict(missing="point", loss="cauchy", scale=-3.0), dict(missing="point", loss="cauchy", scale=float("nan")),
           dict(missing="point", loss="cauchy", scale=float("inf")), dict(missing="point", loss="huber", scale="3"), dict(missing="point", loss="huber", scale=True),
           dict(missing="view", loss="huber", scale=3.0), dict(loss="cauchy", scale=3.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.bundle_adjust_views(calm, rt, C, None, **kw)
        with pytest.raises(ValueError):
            api.BundleAdjustment(calm, rt[0], C[0].T, None, **kw)
    with pytest.raises(ValueError):                                          # the shapes are still checked first
        ctx.bundle_adjust_views(calm, rt, np.zeros((B, N, 5)), None, missing="point", loss="huber", scale=3.0)
