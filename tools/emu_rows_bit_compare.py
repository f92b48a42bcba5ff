#!/usr/bin/env python3
"""Byte comparison of two builds of the lane emulator (tests/emu) on the row kernels, without a GPU.

    python tools/emu_rows_bit_compare.py PARENT.so [RESULT.so]      # RESULT defaults to this tree's tests/emu/_build/libtff_emu.so

PARENT.so is the emulator library of another checkout (g++ -std=c++20 -O1 -pthread -shared -fPIC -Itests/emu -Itft_vs_fund_amd/csrc
tests/emu/emu_lib.cpp, in that checkout).  Scenes: those of tests/test_gpu_rows_boundaries.py (B = 9), and B = 5 and 7 at N = 12 and 27;
kernels: k_linear_tft_pose_rows, k_linear_f_pose_rows and the Gauss-Helmert chain of Ressl (its linear stage runs rows_linear_tft_middle).
Prints one line per cell and the number of differing arrays; exit status 1 when any differs.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from tft_vs_fund_amd.scenes import calm_colmajor, generate_scene_batch   # noqa: E402
from test_gpu_rows_boundaries import NS, boundary_scene                  # noqa: E402


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def run(lib, kernel, C, CalM):
    B, N = C.shape[0], C.shape[1]
    calm = calm_colmajor(CalM)
    o = dict(Rt2=np.zeros((B, 12)), Rt3=np.zeros((B, 12)), T=np.zeros((B, 27)), Rec=np.zeros((B, N, 3)),
             it=np.zeros(B, dtype=np.int32), st=np.ones(B, dtype=np.int32))
    head = (_p(C), _p(calm), ctypes.c_long(0), ctypes.c_long(B), ctypes.c_int(N), ctypes.c_int(0))
    outs = (_p(o["Rt2"]), _p(o["Rt3"]), _p(o["T"]), _p(o["Rec"]), _p(o["it"]), _p(o["st"]))
    if kernel == "ressl":
        lib.emu_gh_wg_pose(ctypes.c_int(0), *head, *outs)
    else:
        getattr(lib, kernel)(*head, *outs, None)
    return o


def main():
    from emu import emu_build
    parent = ctypes.CDLL(os.path.abspath(sys.argv[1]))
    result = ctypes.CDLL(os.path.abspath(sys.argv[2])) if len(sys.argv) > 2 else emu_build.load()
    cells = [("boundary", 9, N, boundary_scene(N)) for N in NS]
    for B in (5, 7):
        for N in (12, 27):
            C, CalM, _, _ = generate_scene_batch(B, N, noise=1.0, seed=4300 + 10 * B + N)
            cells.append(("extra", B, N, (C, CalM)))
    different = compared = 0
    for name, B, N, (C, CalM) in cells:
        for kernel in ("emu_linear_tft_pose_rows", "emu_linear_f_pose_rows", "ressl"):
            if kernel == "ressl" and N not in (12, 27, 200):
                continue                                         # (the slow chain: the sizes of the new tests only)
            a, b = run(parent, kernel, C, CalM), run(result, kernel, C, CalM)
            bad = [k for k in a if a[k].tobytes() != b[k].tobytes()]
            compared += len(a); different += len(bad)
            print("%-9s B=%d N=%-4d %-26s status0=%d/%d  %s" % (name, B, N, kernel, int((b["st"] == 0).sum()), B,
                                                            "byte-identical" if not bad else "DIFFERENT: " + ",".join(bad)))
    print("arrays compared: %d, different: %d" % (compared, different))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
