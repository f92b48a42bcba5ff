#!/usr/bin/env python3
"""Records tests/golden/rows_diet_parent.npz, the bit pin of tests/test_gpu_rows_diet.py, on the GPU:

    python tools/record_rows_diet.py LIBTFTFUND.so [out.npz]

The library is the PARENT commit's (bash tools/build_ab_baseline.sh <commit> P builds tools/ab_libs/libtftfund_P.so), never the code under test: it
has to be named.  Nothing is written unless every triplet of every cell has status 0.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rows_diet_cases as cases         # noqa: E402
from tft_vs_fund_amd import api         # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
lib = os.path.abspath(sys.argv[1])
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "rows_diet_parent.npz")
ctx = api.Context(0, lib_path=lib)
ctx.set_rows(1)                             # the row kernels at any batch size, as the test's context
arrays = cases.record_pin(ctx)
failed = 0
for k in sorted(arrays):
    if k.endswith("/status"):
        failed += int((arrays[k] != 0).sum())
        print("%-50s status 0 on %d of %d" % (k, int((arrays[k] == 0).sum()), arrays[k].size))
if failed:
    sys.exit("%d triplets without status 0: choose other seeds (tests/rows_diet_cases.py)" % failed)
np.savez(out, **arrays)
print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
