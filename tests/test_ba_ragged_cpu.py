"""Ragged BundleAdjustment, the parts that need no GPU: the header, the library and the binding agree on the new symbols; the launch classes are ordered;
the Python wrapper refuses malformed arguments before it enters the library."""
import os
import re

import numpy as np
import pytest

from tft_vs_fund_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tff_bundle_adjust_ragged_dev", "tff_bundle_adjust_ragged_host", "tff_bundle_adjust_ragged_class_bounds")


def _header():
    with open(os.path.join(ROOT, "include", "tftfund.h")) as f:
        return f.read()


def test_header_library_and_binding_agree():
    from tft_vs_fund_amd.build import build_library
    build_library()
    lib = api.load_library()
    h = _header()
    declared = set(re.findall(r"\b(tff_[a-z0-9_]+)\s*\(", h))
    for name in NEW:
        assert name in declared and name in api.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
    assert declared == set(api.EXPORTED_SYMBOLS)
    assert int(re.search(r"#define TFF_ST_TOO_LARGE (\d+)", h).group(1)) == api.ST_TOO_LARGE == 7
    assert int(re.search(r"#define TFF_BA_MAX_N (\d+)", h).group(1)) == api.BA_MAX_N
    assert int(re.search(r"#define TFF_OPT_BA_CLASSES (\d+)", h).group(1)) == api.TFF_OPT_BA_CLASSES
    # the host entry point is the device one without n_total
    dev = re.search(r"int tff_bundle_adjust_ragged_dev\((.*?)\);", h, re.S).group(1)
    host = re.search(r"int tff_bundle_adjust_ragged_host\((.*?)\);", h, re.S).group(1)
    names = lambda sig: [re.sub(r".*[ *]", "", a.strip()) for a in sig.split(",")]
    assert [a for a in names(dev) if a != "n_total"] == names(host)
    assert len(lib.tff_bundle_adjust_ragged_dev.argtypes) == len(names(dev)) and len(lib.tff_bundle_adjust_ragged_host.argtypes) == len(names(host))


def test_class_bounds():
    b = api.ba_ragged_class_bounds()
    assert len(b) == 3 and 0 < b[0] < b[1] < b[2] == api.BA_MAX_N
    # the LDS need is affine in N, 48 bytes per correspondence: the limits 40, 80, 160 KiB are 40 and 80 KiB apart, 853.3 and 1706.7 matches
    assert b[1] - b[0] in (853, 854) and b[2] - b[1] in (1706, 1707)
    h = _header()
    fixed = int(re.search(r"needs ([\d ]+) \+ 48 m bytes of LDS", h).group(1).replace(" ", ""))
    for bound, kib in zip(b, (40, 80, 160)):
        assert fixed + 48 * bound <= kib * 1024 < fixed + 48 * (bound + 1)


class _NoLibrary:
    """a Context whose library is never to be entered"""
    def __getattr__(self, name):
        raise AssertionError("the library was entered: %s" % name)


def _ctx():
    ctx = api.Context.__new__(api.Context)
    ctx.lib = _NoLibrary(); ctx.handle = None; ctx.device = 0
    return ctx


def test_wrapper_refuses_malformed_numpy_arguments_before_the_library():
    ctx = _ctx()
    C = np.zeros((30, 6)); CalM = np.zeros((9, 3)); R = np.zeros((2, 3, 4))
    good = np.array([0, 10, 30], dtype=np.int64)
    for off in (np.array([0, 20, 10]), np.array([-1, 10, 30]), np.array([0.0, 10.0, 30.0]), np.array([[0, 10, 30]]), np.array([0, 10, 31])):
        with pytest.raises(ValueError):
            ctx.bundle_adjust_ragged(CalM, R, R, C, off)
    for mask in (np.ones(29, dtype=np.uint8), np.ones((30, 1), dtype=np.uint8)):
        with pytest.raises(ValueError):
            ctx.bundle_adjust_ragged(CalM, R, R, C, good, mask=mask)
    for r2, r3 in ((np.zeros((3, 3, 4)), R), (R, np.zeros((2, 4, 3))), (np.zeros((2, 12)), R)):
        with pytest.raises(ValueError):
            ctx.bundle_adjust_ragged(CalM, r2, r3, C, good)
    with pytest.raises(ValueError):
        ctx.bundle_adjust_ragged(CalM, R, R, C, good, reconst0=np.zeros((29, 3)))
    with pytest.raises(ValueError):
        ctx.bundle_adjust_ragged(np.zeros((3, 9, 3)), R, R, C, good)
    with pytest.raises(ValueError):
        ctx.bundle_adjust_ragged(CalM, R, R, np.zeros((30, 5)), good)
