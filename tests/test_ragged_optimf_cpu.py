"""
Ragged OptimFPoseEstimation, the part that needs no GPU: tff_optim_f_ragged_bounds is declared, exported and consistent with the header's documented
form of the two bounds; the ragged entry points refuse a null context for method 7; robust_pose_scenes checks `refine` before it touches a device.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tft_vs_fund_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024


def _lds_bytes(F, n, staged):
    """include/tftfund.h: optimf_refine_lds_bytes(n, staged) = 8 (F + 4 n + 2 + (staged ? 6 n : 0))"""
    return 8 * (F + 4 * n + 2 + (6 * n if staged else 0))


def test_bounds_are_exported_and_follow_the_documented_form():
    header = open(os.path.join(ROOT, "include", "tftfund.h")).read()
    assert re.search(r"int\s+tff_optim_f_ragged_bounds\s*\(\s*int32_t\s+bounds\[2\]\s*\)", header)
    assert "tff_optim_f_ragged_bounds" in api.EXPORTED_SYMBOLS
    lib = api.load_library()
    assert lib.tff_optim_f_ragged_bounds(None) == -10001
    S, L = api.optim_f_ragged_bounds()
    assert 0 < S < L
    # the fixed part F is not published: the two bounds must be explained by ONE F, S by the staged form at eight wavefronts per CU (160 KiB / 8 each,
    # 512 bytes of allowance), L by the unstaged form at the same occupancy
    fits_s = lambda F, n: _lds_bytes(F, n, True) + 512 <= LDS_LIMIT // 8
    fits_l = lambda F, n: LDS_LIMIT // (_lds_bytes(F, n, False) + 512) >= 8
    Fs = [F for F in range(0, 4096) if fits_s(F, S) and not fits_s(F, S + 1) and fits_l(F, L) and not fits_l(F, L + 1)]
    assert Fs, (S, L)
    # the kernel's fixed part: OptimFRefineLds (10 + 18 + 12 + 12 doubles) + OptimFLds (10 + 12 + 56 + 11 * 12), the latter rounded up to even
    F = (10 + 18 + 12 + 12) + ((10 + 12 + 56 + 132 + 1) & ~1)
    assert F in Fs, (F, Fs[0], Fs[-1])
    assert "OptimFPoseEstimation" in api.RAGGED_METHODS


def test_null_context_is_refused_for_optim_f():
    lib = api.load_library()
    z = np.zeros(8)
    off = np.zeros(2, dtype=np.int64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.tff_pose_batch_ragged_dev(None, 7, p(z), p(off), 0, p(z), 0, 1, p(z), p(z), p(z), None, None, None) == -10001
    assert lib.tff_pose_batch_ragged_host(None, 7, p(z), p(off), p(z), 0, 1, p(z), p(z), p(z), None, None, None) == -10001
    assert b"null context" in lib.tff_last_error()


def test_refine_is_checked_before_a_device_is_touched():
    ctx = api.Context.__new__(api.Context)                                     # no tff_ctx: any use of the library would fail on the missing handle
    scenes = np.zeros((20, 6)); off = np.array([0, 20], dtype=np.int64); calm = np.zeros((9, 3))
    for bad in ("ResslTFTPoseEstimation", "PiPoseEstimation", "nonsense"):
        with pytest.raises(ValueError, match="LinearTFTPoseEstimation, LinearFPoseEstimation, OptimFPoseEstimation"):
            ctx.robust_pose_scenes("LinearTFTPoseEstimation", scenes, off, calm, 10, 4.0, refine=bad)
