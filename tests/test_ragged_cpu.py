"""Ragged batches without a GPU: the packed layout (api.pack_ragged), host-side offset validation, and the C ABI declarations."""
import os
import re

import numpy as np
import pytest

from tft_vs_fund_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_ragged_layout():
    rng = np.random.default_rng(3)
    items = [rng.standard_normal((n, 6)) for n in (5, 0, 12, 1, 0, 7)]
    corresp, offsets = api.pack_ragged(items)
    assert corresp.dtype == np.float64 and corresp.flags["C_CONTIGUOUS"] and corresp.shape == (25, 6)
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 5, 5, 17, 18, 18, 25]
    for b, x in enumerate(items):
        assert np.array_equal(corresp[offsets[b]:offsets[b + 1]], x)
    assert api.check_offsets(offsets) == 12
    c0, o0 = api.pack_ragged([])
    assert c0.shape == (0, 6) and o0.tolist() == [0] and api.check_offsets(o0) == 0
    with pytest.raises(ValueError):
        api.pack_ragged([np.zeros((3, 5))])


def test_check_offsets_refuses_malformed():
    with pytest.raises(ValueError, match="decrease"):
        api.check_offsets(np.array([0, 4, 3, 9]))
    with pytest.raises(ValueError):
        api.check_offsets(np.array([-1, 4]))
    with pytest.raises(ValueError):
        api.check_offsets(np.array([0.0, 4.0]))
    with pytest.raises(ValueError):
        api.check_offsets(np.zeros((2, 2), dtype=np.int64))


def test_ragged_symbols_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tftfund.h")).read(), flags=re.S)
    for name in ("tff_pose_batch_ragged_dev", "tff_pose_batch_ragged_host"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in api.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+TFF_ST_BAD_OFFSETS\s+6\b", open(os.path.join(ROOT, "include", "tftfund.h")).read())
    assert api.ST_BAD_OFFSETS == 6
    assert set(api.RAGGED_METHODS) <= set(api.METHOD_IDS)


def test_ragged_entry_points_load_and_refuse_without_device():
    """The library exports the ragged entry points; with no context they fail with TFF_E_INVALID instead of computing anything."""
    from tft_vs_fund_amd.build import build_library
    build_library()
    lib = api.load_library()
    assert lib.tff_version() >= 101
    off = np.array([0, 8], dtype=np.int64)
    rc = lib.tff_pose_batch_ragged_host(None, 0, None, off.ctypes.data, None, 0, 1, None, None, None, None, None, None)
    assert rc == -10001
    rc = lib.tff_pose_batch_ragged_dev(None, 0, None, None, 8, None, 0, 1, None, None, None, None, None, None)
    assert rc == -10001


def test_pose_entry_points_refuse_a_null_context():
    """Every `_dev`, `_host` and `_debug_dev` pose entry point answers a null context with TFF_E_INVALID ("null context"), whatever its route
    selection would read from the context."""
    from tft_vs_fund_amd.build import build_library
    build_library()
    lib = api.load_library()
    x = np.zeros(64)
    d = x.ctypes.data
    called = 0
    for stem in api.POSE_METHODS.values():
        for suffix, extra in (("_dev", ()), ("_host", ()), ("_debug_dev", (d,))):
            if stem + suffix not in api.EXPORTED_SYMBOLS or stem + suffix == "tff_pi_pose_batch_debug_dev":   # (its own signature: below)
                continue
            rc = getattr(lib, stem + suffix)(None, d, d, 0, 1, 8, d, d, d, None, None, None, *extra)
            assert rc == -10001 and lib.tff_last_error() == b"null context", stem + suffix
            called += 1
    assert called == 8 + 8 + 5
    for collinear in (0, 1):
        assert lib.tff_pi_pose_batch_debug_dev(None, collinear, d, d, 0, 1, 8, d, d, d, None, None, None, None, None) == -10001
        assert lib.tff_last_error() == b"null context"
