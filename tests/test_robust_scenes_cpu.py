"""
Robust estimation for a batch of scenes, the part that needs no GPU: the three entry points' presence in the header, in api.EXPORTED_SYMBOLS and in
the built library, the version, and the Python wrappers' argument errors, which are raised before the library is entered (the wrappers are called on
an object that has no library and no context: reaching for either would be an AttributeError, not the ValueError asked for).
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tft_vs_fund_amd import api
from tft_vs_fund_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tff_robust_pose_scenes_dev", "tff_robust_pose_scenes_host", "tff_inlier_count_scenes_dev"]
CALM = np.tile(np.diag([800.0, 800.0, 1.0]), (3, 1))


class _NoLibrary(api.Context):
    """the wrappers of Context without a context behind them"""

    def __init__(self):
        self.device = 0

    def __del__(self):
        pass


def test_entry_points_declared_listed_and_exported():
    txt = open(os.path.join(ROOT, "include", "tftfund.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(tff_[a-z0-9_]+)\s*\(", txt))
    build_library()
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in api.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.tff_version() >= 103


def test_entry_points_refuse_a_null_context():
    build_library()
    lib = api.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "tff_robust_pose_scenes_dev": (None, 0, p, p, 8, 8, 1, p, 0, 1, 10, 0, 4.0, 4, 1, p, p, p, p, p, p),
        "tff_robust_pose_scenes_host": (None, 0, p, p, 1, p, 0, 1, 10, 0, 4.0, 4, 1, p, p, p, p, p, p),
        "tff_inlier_count_scenes_dev": (None, p, p, 8, 1, p, 0, p, p, 1, 4.0, p),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -10001, name
        assert lib.tff_last_error().decode() == "null context", name


def test_robust_pose_scenes_argument_errors_come_before_the_library():
    ctx = _NoLibrary()
    scenes = np.zeros((20, 6))
    good = np.array([0, 10, 20], dtype=np.int64)
    with pytest.raises(ValueError):
        ctx.robust_pose_scenes("ResslTFTPoseEstimation", scenes, good, CALM, 100, 4.0)          # the method
    with pytest.raises(ValueError):
        ctx.robust_pose_scenes("LinearTFTPoseEstimation", np.zeros((20, 5)), good, CALM, 100, 4.0)   # the shape of the scenes
    with pytest.raises(ValueError):
        ctx.robust_pose_scenes("LinearTFTPoseEstimation", np.zeros(120), good, CALM, 100, 4.0)
    for bad in (np.array([0, 12, 10], dtype=np.int64), np.array([-1, 10, 20], dtype=np.int64), np.array([[0, 10, 20]], dtype=np.int64),
                np.array([0.0, 10.0, 20.0]), np.array([], dtype=np.int64)):
        with pytest.raises(ValueError):
            ctx.robust_pose_scenes("LinearFPoseEstimation", scenes, bad, CALM, 100, 4.0)       # the offsets, through check_offsets
    with pytest.raises(ValueError):
        ctx.robust_pose_scenes("LinearFPoseEstimation", scenes, np.array([0, 10, 21], dtype=np.int64), CALM, 100, 4.0)   # beyond the packed array
    for bad_calm in (np.zeros((3, 3)), np.zeros((3, 9, 3)), np.zeros((2, 3, 9))):
        with pytest.raises(ValueError):
            ctx.robust_pose_scenes("LinearFPoseEstimation", scenes, good, bad_calm, 100, 4.0)  # CalM: (9, 3) or (S, 9, 3)


def test_inlier_count_scenes_argument_errors_come_before_the_library():
    ctx = _NoLibrary()
    scenes = np.zeros((20, 6))
    good = np.array([0, 10, 20], dtype=np.int64)
    Rt = np.zeros((4, 3, 4))
    for bad in (np.array([0, 12, 10], dtype=np.int64), np.array([-1, 10, 20], dtype=np.int64), np.array([0.0, 10.0, 20.0])):
        with pytest.raises(ValueError):
            ctx.inlier_count_scenes(scenes, bad, CALM, Rt, Rt)
    with pytest.raises(ValueError):
        ctx.inlier_count_scenes(np.zeros((20, 5)), good, CALM, Rt, Rt)
    with pytest.raises(ValueError):
        ctx.inlier_count_scenes(scenes, good, CALM, np.zeros((4, 4, 3)), Rt)
    with pytest.raises(ValueError):
        ctx.inlier_count_scenes(scenes, good, CALM, np.zeros((3, 3, 4)), np.zeros((3, 3, 4)))   # 3 poses for 2 scenes
    with pytest.raises(ValueError):
        ctx.inlier_count_scenes(scenes, good, CALM, Rt, np.zeros((2, 3, 4)))
    with pytest.raises(ValueError):
        ctx.inlier_count_scenes(scenes, good, np.zeros((3, 9, 3)), Rt, Rt)
