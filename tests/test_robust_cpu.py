"""
Robust estimation, the part that needs no GPU: the sampler's definition (api.sample_indices_reference, the numpy statement of what
tff_sample_indices_dev computes), and the new entry points' presence in the header, in api.EXPORTED_SYMBOLS and in the built library.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tft_vs_fund_amd import api
from tft_vs_fund_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 400), (8, 9), (16, 16), (8, 8), (7, 1400)]
NEW_SYMBOLS = ["tff_sample_indices_dev", "tff_inlier_mask_batch_dev", "tff_robust_pose_dev", "tff_robust_pose_host"]


def test_sampler_known_answer():
    out = api.sample_indices_reference(1234, 0, 2, 7, 400)
    assert out.dtype == np.int32 and out.shape == (2, 7)
    assert out[0].tolist() == [247, 279, 158, 173, 205, 359, 68]
    assert out[1].tolist() == [203, 236, 320, 382, 155, 282, 100]


@pytest.mark.parametrize("n,Ns", SHAPES)
def test_sampler_rows_distinct_and_in_range(n, Ns):
    out = api.sample_indices_reference(99, 0, 20000, n, Ns)
    assert out.min() >= 0 and out.max() < Ns
    assert (np.diff(np.sort(out, axis=1), axis=1) > 0).all()


def test_sampler_is_counter_based():
    whole = api.sample_indices_reference(5, 0, 1000, 7, 400)
    part = api.sample_indices_reference(5, 400, 600, 7, 400)
    assert np.array_equal(whole[400:], part)
    far = api.sample_indices_reference(5, (1 << 40) + 3, 4, 7, 400)           # a first beyond 2^32
    assert np.array_equal(far[1:], api.sample_indices_reference(5, (1 << 40) + 4, 3, 7, 400))
    assert not np.array_equal(whole, api.sample_indices_reference(6, 0, 1000, 7, 400))   # another seed, other samples


@pytest.mark.parametrize("n,Ns", SHAPES)
def test_sampler_uniform(n, Ns):
    """Every index is drawn m = B n / Ns times on average, a binomial count with standard deviation sqrt(m (1 - n / Ns)); the last position alone
    B / Ns times with sqrt(B / Ns (1 - 1 / Ns)).  Bound: 6 standard deviations (a 2e-9 tail per index, at most 1 400 indices); n = Ns leaves no
    freedom for the whole row (every index exactly B times).  Measured: within 3.5 on all five shapes, both statistics."""
    B = 100000
    out = api.sample_indices_reference(1234, 0, B, n, Ns)
    m = B * n / Ns
    dev = np.abs(np.bincount(out.ravel(), minlength=Ns) - m)
    sd = np.sqrt(m * (1 - n / Ns))
    print("n %d Ns %d: all positions %.2f sd" % (n, Ns, dev.max() / sd if sd else 0.0))
    assert dev.max() <= 6 * sd
    m1 = B / Ns
    dev1 = np.abs(np.bincount(out[:, n - 1], minlength=Ns) - m1)
    sd1 = np.sqrt(m1 * (1 - 1 / Ns))
    print("n %d Ns %d: last position %.2f sd" % (n, Ns, dev1.max() / sd1))
    assert dev1.max() <= 6 * sd1


def test_sampler_rejects_bad_arguments():
    for args in ((0, 0, 1, 0, 10), (0, 0, 1, 17, 100), (0, 0, 1, 7, 6), (0, 0, -1, 7, 10), (0, -1, 1, 7, 10)):
        with pytest.raises(ValueError):
            api.sample_indices_reference(*args)


def test_new_entry_points_declared_listed_and_exported():
    txt = open(os.path.join(ROOT, "include", "tftfund.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(tff_[a-z0-9_]+)\s*\(", txt))
    build_library()
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in api.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.tff_version() >= 102
    assert api.ROBUST_CHUNK >= 1
    assert "tff_repr_error_ragged_dev" not in open(os.path.join(ROOT, "include", "tftfund.h")).read()


def test_new_entry_points_refuse_a_null_context():
    build_library()
    lib = api.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "tff_sample_indices_dev": (None, 1, 0, 1, 7, 400, p),
        "tff_inlier_mask_batch_dev": (None, p, 1, p, p, p, 1, 4.0, p, None),
        "tff_robust_pose_dev": (None, 0, p, 8, p, 1, 10, 0, 4.0, 4, 1, p, p, p, p, p, p),
        "tff_robust_pose_host": (None, 0, p, 8, p, 1, 10, 0, 4.0, 4, 1, p, p, p, p, p, p),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -10001, name
        assert lib.tff_last_error().decode() == "null context", name
