#!/usr/bin/env python3
"""Records tests/golden/rows_lane_roles_parent.npz, the bit pin of tests/test_gpu_rows_lane_roles.py, on the GPU:

    python tools/record_rows_lane_roles.py [libtftfund.so] [out.npz]

With no library the in-tree build is used; tools/build_ab_baseline.sh <commit> <tag> builds another commit's as tools/ab_libs/libtftfund_<tag>.so.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rows_lane_roles_cases as cases   # noqa: E402
from tft_vs_fund_amd import api         # noqa: E402

lib = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "rows_lane_roles_parent.npz")
ctx = api.Context(0, lib_path=lib)
ctx.set_rows(1)                             # the row kernels at any batch size, as the test's context
arrays = cases.record_pin(ctx)
for k in sorted(arrays):
    if k.endswith("/status"):
        print("%-50s status 0 on %d of %d" % (k, int((arrays[k] == 0).sum()), arrays[k].size))
np.savez(out, **arrays)
print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
