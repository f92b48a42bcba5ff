"""
TFF_OPT_SCORE without a GPU: the option's number and TFF_SCORE_UNITS are the same in include/tftfund.h and in tft_vs_fund_amd.api, Context.set_score
refuses an unknown name before it touches the library, and the option added no entry point.
"""
import hashlib
import os
import re

import pytest

from tft_vs_fund_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    m = re.search(r"^#define\s+%s\s+(-?\d+)\b" % name, open(os.path.join(ROOT, "include", "tftfund.h")).read(), flags=re.M)
    assert m, name
    return int(m.group(1))


def test_header_and_api_constants_agree():
    assert _define("TFF_OPT_SCORE") == api.TFF_OPT_SCORE == 13
    assert _define("TFF_SCORE_UNITS") == api.SCORE_UNITS == 64
    numbers = [v for k, v in vars(api).items() if k.startswith("TFF_OPT_")]
    assert len(numbers) == len(set(numbers))                                  # no option number is used twice


def test_set_score_refuses_an_unknown_name_before_the_library():
    ctx = api.Context.__new__(api.Context)                                    # no library, no handle: touching either raises AttributeError
    for bad in ("nonsense", "MSAC", 1, None):
        with pytest.raises(ValueError):
            ctx.set_score(bad)
    with pytest.raises(AttributeError):
        ctx.set_score("msac")                                                 # a known name goes on to the library


def test_no_new_entry_point():
    """the 64 symbols of the library before the option, in their order"""
    assert len(api.EXPORTED_SYMBOLS) == 64
    assert hashlib.sha256("\n".join(api.EXPORTED_SYMBOLS).encode()).hexdigest() == "06f73780337627c34d616ce762c65c6bdc69570f2235a8ac60f395853736d1dd"
