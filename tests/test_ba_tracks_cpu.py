"""
The bundle adjustment over tracks (include/tftfund_tracks.h), the part that needs no GPU: the header, the symbol list and the library agree, the header
compiles as C in either order, the entry points refuse a null context, and the Python wrappers refuse a bad missing= and bad shapes before a device is
touched.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tft_vs_fund_amd import api
from tft_vs_fund_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tff_bundle_adjust_tracks_batch_dev", "tff_bundle_adjust_tracks_batch_host"]


class _NoLibrary(api.Context):
    """the wrappers of Context without a context behind them"""

    def __init__(self):
        self.device = 0

    def __del__(self):
        pass


def test_entry_points_declared_listed_and_exported():
    main = open(os.path.join(ROOT, "include", "tftfund.h")).read()
    tail = main[main.rindex("#ifdef __cplusplus"):]
    assert re.findall(r'^#include "(tftfund_\w+\.h)"', main, flags=re.M).count("tftfund_tracks.h") == 1 and '#include "tftfund_tracks.h"' in tail   # at the end
    txt = open(os.path.join(ROOT, "include", "tftfund_tracks.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tff_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(api.TRACKS_SYMBOLS) == sorted(NEW_SYMBOLS)
    assert not set(api.TRACKS_SYMBOLS) & (set(api.EXPORTED_SYMBOLS) | set(api.ADAPTIVE_SYMBOLS) | set(api.GUIDED_SYMBOLS) | set(api.LOSS_SYMBOLS) | set(api.COV_SYMBOLS))
    # the argument list is that of the whole-view call plus `int32_t* used` before `status`
    views = re.search(r"int tff_bundle_adjust_views_batch_dev\((.*?)\);", main, flags=re.S).group(1)
    tracks = re.search(r"int tff_bundle_adjust_tracks_batch_dev\((.*?)\);", txt, flags=re.S).group(1)
    norm = lambda a: [" ".join(x.split()) for x in a.split(",")]
    assert norm(tracks) == norm(views)[:-1] + ["int32_t* used", "int32_t* status"]
    build_library()
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.tff_version() >= 108


def test_header_compiles_as_c_in_either_order(tmp_path):
    for n, first in enumerate(("tftfund.h", "tftfund_tracks.h")):
        src = tmp_path / ("t%d.c" % n)
        src.write_text('#include "%s"\n#include "tftfund.h"\n#include "tftfund_tracks.h"\n'
                       'int (*p)(tff_ctx*, int32_t, const double*, int64_t, const double*, const double*, int64_t, int32_t, const double*, double*, double*,\n'
                       '         int32_t*, double*, int32_t*, int32_t*) = tff_bundle_adjust_tracks_batch_host;\n' % first)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_entry_points_refuse_a_null_context():
    build_library()
    lib = api.load_library()
    buf = (ctypes.c_double * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in NEW_SYMBOLS:
        assert getattr(lib, name)(None, 3, p, 0, p, p, 1, 8, None, p, p, p, p, p, p) == -10001, name      # TFF_E_INVALID
        assert lib.tff_last_error().decode() == "null context", name


def test_python_argument_errors_come_before_the_library():
    ctx = _NoLibrary()
    M, B, N = 3, 2, 10
    calm = np.tile(np.diag([800.0, 800.0, 1.0]), (M, 1)); rt = np.zeros((B, 3 * M, 4)); C = np.zeros((B, N, 2 * M))
    for missing in ("points", "track", None, 1):
        with pytest.raises(ValueError):
            ctx.bundle_adjust_views(calm, rt, C, None, missing=missing)
        with pytest.raises(ValueError):
            api.BundleAdjustment(calm, rt[0], C[0].T, None, missing=missing)
    bad = [(calm, rt, C[0], None),                                                       # corresp without a batch axis
           (calm, rt, np.zeros((B, N, 5)), None),                                       # an odd number of rows
           (calm, rt, np.zeros((B, N, 14)), None),                                      # seven views
           (calm, rt[:, :6], C, None), (calm, rt[:1], C, None),                         # poses of another M, another B
           (calm[:6], rt, C, None), (np.stack([calm] * 3), rt, C, None),                # calibration of another M, another B
           (calm, rt, C, np.zeros((B, 3, N + 1))), (calm, rt, C, np.zeros((B, N, 3)))]  # reconst0
    for args in bad:
        with pytest.raises(ValueError):
            ctx.bundle_adjust_views(*args, missing="point")
    with pytest.raises(ValueError):
        api.BundleAdjustment(calm, rt[0], C[0].T, np.zeros((3, N + 1)), missing="point")
    with pytest.raises(ValueError):
        api.BundleAdjustment(calm[:6], rt[0], C[0].T, None, missing="point")
