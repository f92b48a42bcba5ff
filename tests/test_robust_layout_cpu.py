"""
The workspace layouts of the robust estimators (csrc/robust_layout.h), no GPU: the header is compiled by g++ alone into a stand-alone program
(tests/emu/layout_probe.cpp) and every region of both workspaces is checked for each size tuple -- it starts on a 256-byte boundary, is disjoint from the
others and lies inside the total -- and the totals are those of the formulas launch_robust_scenes computed before the layouts were described once
(written out below from that source).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")

# (chunk, S, K, n, n_total, copies, adaptive); C = S * K.  copies: 216 bytes with one CalM per scene, 0 with a shared one
CASES = [
    (100, 1, 1, 7, 61, 0, False),            # one scene, one candidate, shared CalM
    (262144, 40, 16, 7, 1600, 216, True),    # a full chunk, per-scene CalM, the rounds' state
    (160, 40, 16, 8, 1600, 0, True),         # adaptive with a shared CalM
    (0, 3, 64, 16, 0, 216, False),           # n_total = 0: no chunk, no flags, no refit batch; K = 64, n = 16
    (768, 3, 4, 16, 221, 216, False),        # odd sizes, n = 16
    (1, 1, 64, 7, 7, 0, True),               # the smallest adaptive call, K = 64, n = 7
]


@pytest.fixture(scope="module")
def probe():
    out_dir = os.path.join(EMU, "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "layout_probe")
    deps = [os.path.join(EMU, "layout_probe.cpp"), os.path.join(CSRC, "robust_layout.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, deps[0]], check=True)
    return exe


def a256(b):
    return (b + 255) & ~255


def regions(case):
    """the bytes of every region, in the order of the structs, from what the region holds"""
    chunk, S, K, n, n_total, copies, adaptive = case
    C = S * K
    rounds = [chunk * 4, S * 8, S * 4] if adaptive else [0, 0, 0]
    hyp = [chunk * 51 * 8, chunk * copies, chunk * 4, chunk * n * 4] + rounds
    cand = [C * 8, C * 51 * 8, C * 51 * 8, (C + 1) * 8, C * 7 * 4, C * n * 4, C * copies, K * n_total, K * n_total * 6 * 8]
    return hyp, cand


def parent_totals(case):
    """hyp_bytes + round_bytes and the carve total of launch_robust_scenes before this header existed"""
    chunk, S, K, n, n_total, copies, adaptive = case
    C = S * K
    hyp_bytes = a256(chunk * 51 * 8) + a256(chunk * copies) + a256(chunk * 4) + a256(chunk * n * 4)
    round_bytes = a256(chunk * 4) + a256(S * 8) + a256(S * 4) if adaptive else 0
    cand = (a256(C * 8) + a256(C * 51 * 8) + a256(C * 51 * 8) + a256((C + 1) * 8) + a256(C * 7 * 4) + a256(C * n * 4) + a256(C * copies)
            + a256(K * n_total) + a256(K * n_total * 6 * 8))
    return hyp_bytes + round_bytes, cand


@pytest.mark.parametrize("case", CASES)
def test_layout(probe, case):
    chunk, S, K, n, n_total, copies, adaptive = case
    r = subprocess.run([probe] + [str(int(v)) for v in (chunk, S, S * K, K, n, n_total, copies, adaptive)], check=True, capture_output=True, text=True)
    hyp, cand = [[int(x) for x in line.split()] for line in r.stdout.strip().split("\n")]
    assert len(hyp) == 8 and len(cand) == 10
    for got, sizes, total in zip((hyp, cand), regions(case), parent_totals(case)):
        starts, end = got[:-1], got[-1]
        assert end == total
        assert all(s % 256 == 0 for s in starts)
        spans = sorted((s, s + b) for s, b in zip(starts, sizes) if b)       # (a region of zero bytes overlaps nothing)
        assert all(0 <= s and e <= end for s, e in spans)
        assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
        assert all(0 <= s <= end for s in starts)
