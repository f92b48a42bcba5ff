"""
The adaptive robust call (a confidence and a cap instead of a fixed number of hypotheses), the part that needs no GPU: the plan of rounds against Python, the
three entry points' presence and their refusal of a null context, and the Python wrappers' argument errors, which are raised before the library is entered
(the wrappers are called on an object that has no library and no context, as in tests/test_robust_scenes_cpu.py).
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tft_vs_fund_amd import api
from tft_vs_fund_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tff_robust_pose_scenes_adaptive_dev", "tff_robust_pose_scenes_adaptive_host", "tff_robust_round_plan"]
CALM = np.tile(np.diag([800.0, 800.0, 1.0]), (3, 1))


class _NoLibrary(api.Context):
    """the wrappers of Context without a context behind them"""

    def __init__(self):
        self.device = 0

    def __del__(self):
        pass


def _plan(c, n_hyp, first):
    ends = []
    r = 1
    while True:
        e = min(n_hyp, first << (r - 1))
        ends.append(e)
        if e == n_hyp:
            return ends, [-math.expm1(math.log1p(-c) / e) for e in ends]
        r += 1


@pytest.mark.parametrize("c, n_hyp, first", [
    (0.99, 65536, 256),              # a power of two: 9 rounds
    (0.99, 2049, 64),                # a cap that is no power of two: the last round has 1 025 hypotheses
    (0.999, 1000, 1000),             # first_round = n_hyp: one round
    (0.5, 100, 256),                 # first_round > n_hyp: one round of n_hyp
    (0.95, 1, 4),
    (0.99, (4 << 30) - 5, 4),        # 31 rounds
    (0.99, 4 << 30, 4),              # 31 rounds, the last one ending exactly at the cap
    (1e-9, 10 ** 6, 12), (1 - 1e-12, 10 ** 6, 12),
])
def test_round_plan_against_python(c, n_hyp, first):
    build_library()
    ends, qmin = api.round_plan(c, n_hyp, first)
    ref_e, ref_q = _plan(c, n_hyp, first)
    assert ends.dtype == np.int64 and ends.tolist() == ref_e
    assert qmin.shape == ends.shape
    for got, want in zip(qmin, ref_q):
        assert abs(got - want) <= 1e-15 * abs(want), (got, want)
    assert ends[-1] == n_hyp and (np.diff(ends) > 0).all() and (np.diff(qmin) < 0).all()
    if (c, n_hyp, first) in ((0.99, (4 << 30) - 5, 4), (0.99, 4 << 30, 4)):
        assert len(ends) == 31


def test_round_plan_refusals():
    build_library()
    lib = api.load_library()
    ends = (ctypes.c_int64 * 32)(); qmin = (ctypes.c_double * 32)(); rounds = ctypes.c_int32(7)
    pe, pq, pr = (ctypes.cast(x, ctypes.c_void_p) for x in (ends, qmin, ctypes.pointer(rounds)))
    for c, n_hyp, first in ((0.0, 100, 4), (1.0, 100, 4), (-0.5, 100, 4), (float("nan"), 100, 4), (0.9, 0, 4), (0.9, 100, 0), (0.9, 100, 2), (0.9, 100, 6),
                            (0.9, 100, -4), (0.9, 1 << 40, 4)):                 # the last one: more than 32 rounds
        assert lib.tff_robust_round_plan(c, n_hyp, first, pe, pq, pr) == -10001, (c, n_hyp, first)
    assert lib.tff_robust_round_plan(0.9, 100, 4, None, pq, pr) == -10001
    assert lib.tff_robust_round_plan(0.9, (4 << 31), 4, pe, pq, pr) == 0 and rounds.value == 32
    for bad in ((0.0, 100, 4), (1.0, 100, 4), (float("nan"), 100, 4), (0.9, 100, 6), (0.9, 100, 0), (0.9, 100, 4.5), (0.9, 0, 4), (0.9, 10.5, 4)):
        with pytest.raises(ValueError):
            api.round_plan(*bad)


def test_entry_points_declared_listed_and_exported():
    """the new entry points live in include/tftfund_adaptive.h, which tftfund.h includes; api.ADAPTIVE_SYMBOLS lists exactly what it declares"""
    main = open(os.path.join(ROOT, "include", "tftfund.h")).read()
    assert re.search(r'^#include "tftfund_adaptive.h"', main, flags=re.M)
    txt = open(os.path.join(ROOT, "include", "tftfund_adaptive.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tff_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(api.ADAPTIVE_SYMBOLS) == sorted(NEW_SYMBOLS)
    assert not set(api.ADAPTIVE_SYMBOLS) & set(api.EXPORTED_SYMBOLS)
    build_library()
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.tff_version() >= 104


def test_headers_compile_as_c_in_either_order(tmp_path):
    for n, first in enumerate(("tftfund.h", "tftfund_adaptive.h")):
        src = tmp_path / ("t%d.c" % n)
        src.write_text('#include "%s"\n#include "tftfund.h"\nint (*p)(double, int64_t, int32_t, int64_t*, double*, int32_t*) = tff_robust_round_plan;\n' % first)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_entry_points_refuse_a_null_context():
    build_library()
    lib = api.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "tff_robust_pose_scenes_adaptive_dev": (None, 0, p, p, 8, 8, 1, p, 0, 1, 10, 0, 4.0, 4, 1, 0.99, 4, p, p, p, p, p, p, p),
        "tff_robust_pose_scenes_adaptive_host": (None, 0, p, p, 1, p, 0, 1, 10, 0, 4.0, 4, 1, 0.99, 4, p, p, p, p, p, p, p),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -10001, name
        assert lib.tff_last_error().decode() == "null context", name


def test_adaptive_argument_errors_come_before_the_library():
    ctx = _NoLibrary()
    scenes = np.zeros((20, 6))
    good = np.array([0, 10, 20], dtype=np.int64)
    for conf, first in ((0.0, 256), (1.0, 256), (1.5, 256), (-0.1, 256), (float("nan"), 256), (0.99, 0), (0.99, 2), (0.99, 6), (0.99, -8), (0.99, 8.5)):
        with pytest.raises(ValueError):
            ctx.robust_pose_scenes("LinearTFTPoseEstimation", scenes, good, CALM, 100, 4.0, confidence=conf, first_round=first)
        with pytest.raises(ValueError):
            ctx.robust_pose("LinearFPoseEstimation", scenes, CALM, 100, 4.0, confidence=conf, first_round=first)
    with pytest.raises(ValueError):
        ctx.robust_pose_scenes("ResslTFTPoseEstimation", scenes, good, CALM, 100, 4.0, confidence=0.99)          # the method
    with pytest.raises(ValueError):
        ctx.robust_pose("ResslTFTPoseEstimation", scenes, CALM, 100, 4.0, confidence=0.99)
    with pytest.raises(ValueError):
        ctx.robust_pose_scenes("LinearTFTPoseEstimation", np.zeros((20, 5)), good, CALM, 100, 4.0, confidence=0.99)   # the shape of the scenes
    with pytest.raises(ValueError):
        ctx.robust_pose("LinearTFTPoseEstimation", np.zeros((20, 5)), CALM, 100, 4.0, confidence=0.99)
    with pytest.raises(ValueError):
        ctx.robust_pose("LinearTFTPoseEstimation", scenes, np.zeros((3, 3)), 100, 4.0, confidence=0.99)              # CalM
    with pytest.raises(ValueError):
        ctx.robust_pose("LinearTFTPoseEstimation", scenes, CALM, 100, 4.0, confidence=0.99, refine="NoSuchMethod")
    for bad in (np.array([0, 12, 10], dtype=np.int64), np.array([-1, 10, 20], dtype=np.int64), np.array([0, 10, 21], dtype=np.int64)):
        with pytest.raises(ValueError):
            ctx.robust_pose_scenes("LinearFPoseEstimation", scenes, bad, CALM, 100, 4.0, confidence=0.99)          # the offsets
    with pytest.raises(ValueError):
        ctx.robust_pose_scenes("LinearFPoseEstimation", scenes, good, CALM, 100, 4.0, confidence=0.99, refine="PiPoseEstimation")


def test_adaptive_stop_is_the_rule():
    """the numpy twin on hand-made cases: I >= 1, q = w^n by repeated multiplication, >= (equality stops); MSAC divides the score by 64 first"""
    w = np.float64(3) / np.float64(10)
    q = w
    for _ in range(6):
        q = q * w
    assert api.adaptive_stop(3, 10, 7, q) and not api.adaptive_stop(3, 10, 7, np.nextafter(q, 1.0))
    assert not api.adaptive_stop(0, 10, 7, 0.0) and not api.adaptive_stop(-1, 10, 7, 0.0)
    assert api.adaptive_stop(10, 10, 8, 1.0)
    assert api.adaptive_stop(3 * 64 + 63, 10, 7, q, msac=True) and not api.adaptive_stop(3 * 64 - 1, 10, 7, q, msac=True)
    assert not api.adaptive_stop(63, 10, 7, 0.0, msac=True)
