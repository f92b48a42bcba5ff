"""
Quality-guided (PROSAC) sampling, the part that needs no GPU: the numpy twins that define it (api.guided_pool_ends, api.sample_indices_guided_reference)
against their stated properties and against a scalar pure-Python restatement of include/tftfund_guided.h; the header, the symbol list and the library;
the Python wrappers' argument errors, raised before the library is entered; and the seeds of the GPU suite's end-to-end case.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tft_vs_fund_amd import api
from tft_vs_fund_amd.build import build_library

import guided_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tff_robust_pose_scenes_guided_dev", "tff_robust_pose_scenes_guided_host", "tff_sample_indices_guided_dev"]
CALM = np.tile(np.diag([800.0, 800.0, 1.0]), (3, 1))
CASES = [(7, 7, 1), (8, 8, 50), (61, 7, 200000), (400, 8, 64), (5000, 7, 200000)]
M64 = (1 << 64) - 1


class _NoLibrary(api.Context):
    """the wrappers of Context without a context behind them"""

    def __init__(self):
        self.device = 0

    def __del__(self):
        pass


# ---- the definition once more, scalar, in pure Python -------------------------------------------------------------------------------------------------
def _splitmix(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _draw(seed, h, n, Ns):
    """the uniform sampler (csrc/robust_kernel.h::sample_draw) for one hypothesis"""
    key = _splitmix((seed ^ ((h * 0xD1342543DE82EF95) & M64)) & M64)
    pos, val, out = [], [], []
    for i in range(n):
        u = _splitmix((key + i) & M64) >> 32
        r = i + ((u * (Ns - i)) >> 32)
        vr, vi = r, i
        for p, v in zip(pos, val):
            if p == r:
                vr = v
            if p == i:
                vi = v
        out.append(vr)
        pos.append(r); val.append(vi)
    return out


def _T(n, N, m, G):
    T = float(G)
    for i in range(m):
        T = T * float(n - i)
        T = T / float(N - i)
    return T


def _ends(N, m, G):
    ends = [0] * (N + 1)
    ends[m] = 1
    for n in range(m, N):
        ends[n + 1] = ends[n] + int(math.ceil(_T(n + 1, N, m, G) - _T(n, N, m, G)))
    return ends


def _row(seed, h, m, order, ends):
    N = len(order)
    t = h + 1
    if t > ends[N]:
        ranks = _draw(seed, h, m, N)
    else:
        n = next(k for k in range(m, N + 1) if ends[k] >= t)
        ranks = (_draw(seed, h, m - 1, n - 1) if m > 1 else []) + [n - 1]
    idx = [int(order[r]) for r in ranks]
    return [-1] * m if any(i < 0 or i >= N for i in idx) else idx


@pytest.mark.parametrize("N, m, G", CASES)
def test_twins_against_the_scalar_definition(N, m, G):
    ends = api.guided_pool_ends(N, m, G)
    ref = _ends(N, m, G)
    assert ends.dtype == np.int32 and ends.tolist() == ref
    order = np.random.default_rng(N + m).permutation(N).astype(np.int32)
    last = ref[N]
    # hypotheses at the start, around the end of the table, and far beyond it
    firsts = sorted({0, max(0, last - 30), last + 1000, (1 << 32) - 3} | ({max(0, last // 2 - 10)} if N > m else set()))
    for first in firsts:
        got = api.sample_indices_guided_reference(12345, first, 40, m, order, G)
        assert got.dtype == np.int32 and got.shape == (40, m)
        for b in range(40):
            assert got[b].tolist() == _row(12345, first + b, m, order, ref), (first, b)


@pytest.mark.parametrize("N, m, G", CASES)
def test_properties_of_the_twins(N, m, G):
    ends = api.guided_pool_ends(N, m, G).astype(np.int64)
    assert (ends[:m] == 0).all() and ends[m] == 1 and (np.diff(ends[m:]) >= 0).all() and ends[N] <= G + N
    order = np.random.default_rng(3).permutation(N).astype(np.int32)
    B = int(min(ends[N], 3000)) + 50
    rows = api.sample_indices_guided_reference(9, 0, B, m, order, G)
    assert sorted(rows[0].tolist()) == sorted(order[:m].tolist()) and rows[0, -1] == order[m - 1]   # h = 0: the ranks 0 .. m-1 through order, rank m-1 last
    assert all(len(set(r)) == m for r in rows.tolist())                       # distinct, as order is a permutation
    assert rows.min() >= 0 and rows.max() < N
    # each row's last entry has rank pool - 1; rows beyond the table are the uniform sampler through order
    rank_of = np.empty(N, dtype=np.int64); rank_of[order] = np.arange(N)
    pool = api.guided_pool(ends, m, np.arange(1, B + 1))
    for h in range(B):
        if pool[h]:
            assert m <= pool[h] <= N and ends[pool[h]] >= h + 1 and (pool[h] == m or ends[pool[h] - 1] < h + 1)
            assert rank_of[rows[h, -1]] == pool[h] - 1 and rank_of[rows[h, :-1]].max(initial=-1) < pool[h] - 1
        else:
            assert h + 1 > ends[N]
    first = int(ends[N])                                                      # h >= ends[N], i.e. t > ends[N]
    tail = api.sample_indices_guided_reference(9, first, 200, m, order, G)
    assert np.array_equal(tail, order[api.sample_indices_reference(9, first, 200, m, N)])
    far = api.sample_indices_guided_reference(9, (1 << 32) - 3, 50, m, order, G)
    assert np.array_equal(far, order[api.sample_indices_reference(9, (1 << 32) - 3, 50, m, N)])


def test_a_scene_of_one_sample_is_the_top_m_then_uniform():
    for N, G in ((7, 1), (7, 1000), (8, 50)):
        order = np.random.default_rng(N).permutation(N).astype(np.int32)
        ends = api.guided_pool_ends(N, N, G)
        assert ends[N] == 1
        rows = api.sample_indices_guided_reference(4, 0, 30, N, order, G)
        assert sorted(rows[0].tolist()) == list(range(N)) and rows[0, -1] == order[N - 1]     # the top m = all of them, rank N-1 last
        assert np.array_equal(rows[1:], order[api.sample_indices_reference(4, 1, 29, N, N)])


def test_out_of_range_entries_duplicates_and_refusals():
    order = np.arange(20, dtype=np.int32)[::-1].copy()
    clean = api.sample_indices_guided_reference(1, 0, 300, 7, order, 100)
    for bad_value in (-1, 20, 1 << 30):
        bad = order.copy(); bad[5] = bad_value
        got = api.sample_indices_guided_reference(1, 0, 300, 7, bad, 100)
        hit = (clean == order[5]).any(axis=1)
        assert 0 < hit.sum() < 300 and (got[hit] == -1).all() and np.array_equal(got[~hit], clean[~hit])
    dup = np.zeros(20, dtype=np.int32)                                        # duplicates are no error: degenerate samples
    assert (api.sample_indices_guided_reference(1, 0, 10, 7, dup, 100) == 0).all()
    for growth in (0, -1, api.GUIDED_MAX_GROWTH + 1, 1 << 40, 2.5):
        with pytest.raises(ValueError):
            api.guided_pool_ends(20, 7, growth)
        with pytest.raises(ValueError):
            api.sample_indices_guided_reference(1, 0, 10, 7, order, growth)
    assert api.GUIDED_MAX_GROWTH == 2 ** 31 - 2 ** 25
    api.guided_pool_ends(20, 7, api.GUIDED_MAX_GROWTH)
    for Ns, n in ((6, 7), (20, 0), (20, 17)):
        with pytest.raises(ValueError):
            api.guided_pool_ends(Ns, n, 10)
    with pytest.raises(ValueError):
        api.sample_indices_guided_reference(1, 0, 10, 7, order.astype(np.float64), 100)
    assert api.guided_pool_ends(1 << 24, 16, api.GUIDED_MAX_GROWTH).astype(np.int64)[-1] <= api.GUIDED_MAX_GROWTH + (1 << 24) < 2 ** 31


def test_order_from_quality_is_the_stated_rule():
    off = np.array([2, 7, 7, 12], dtype=np.int64)                             # a gap in front, an empty scene, three entries behind
    # whatever the entries outside the scenes hold -- the lowest, NaN, the highest, a value in between -- they take no part in any scene's ranking
    for front, back in (([-9.0, np.nan], [5.0, 5.0, 5.0]), ([9.0, 9.0], [np.nan, -7.0, 99.0]), ([2.5, -np.inf], [np.inf, 0.0, 2.0])):
        q = np.array(front + [0.5, 2.0, np.nan, 2.0, -1.0, 3.0, 3.0, 1.0, np.inf, -np.inf] + back)
        order = api.order_from_quality(q, off)
        assert order.dtype == np.int32 and order.shape == (15,)
        assert order[2:7].tolist() == [1, 3, 0, 4, 2]                         # 2.0 (first), 2.0 (second: stable), 0.5, -1.0, NaN last
        assert order[7:12].tolist() == [3, 0, 1, 2, 4]                        # inf, 3.0, 3.0, 1.0, -inf
        assert order[:2].tolist() == [-1, -1] and order[12:].tolist() == [-1, -1, -1]   # no scene: no rank
    assert api.order_from_quality([-5, -6, 3, 1, 2, 0, 4, 9, 8, 7, 6, 5], [2, 7, 12]).tolist() == [-1, -1, 4, 0, 2, 1, 3, 0, 1, 2, 3, 4]
    for trial in range(20):                                                   # against a per-scene argsort, random offsets with a gap and a tail
        rng = np.random.default_rng(trial)
        cuts = np.sort(rng.integers(0, 40, 5)).astype(np.int64)
        q = np.round(rng.normal(0, 1, 45), 1)
        q[rng.integers(0, 45, 3)] = np.nan
        got = api.order_from_quality(q, cuts)
        want = np.full(45, -1)
        for s in range(4):
            seg = np.where(np.isnan(q[cuts[s]:cuts[s + 1]]), -np.inf, q[cuts[s]:cuts[s + 1]])
            want[cuts[s]:cuts[s + 1]] = np.argsort(-seg, kind="stable")
        assert got.tolist() == want.tolist(), trial
    ties = np.zeros(6)
    assert api.order_from_quality(ties, np.array([0, 6])).tolist() == [0, 1, 2, 3, 4, 5]


# ---- header, symbols, library ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_and_exported():
    main = open(os.path.join(ROOT, "include", "tftfund.h")).read()
    assert re.search(r'^#include "tftfund_guided.h"', main, flags=re.M)
    txt = open(os.path.join(ROOT, "include", "tftfund_guided.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tff_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(api.GUIDED_SYMBOLS) == sorted(NEW_SYMBOLS)
    assert not set(api.GUIDED_SYMBOLS) & (set(api.EXPORTED_SYMBOLS) | set(api.ADAPTIVE_SYMBOLS))
    build_library()
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.tff_version() >= 105


def test_header_compiles_as_c_in_either_order(tmp_path):
    for n, first in enumerate(("tftfund.h", "tftfund_guided.h")):
        src = tmp_path / ("t%d.c" % n)
        src.write_text('#include "%s"\n#include "tftfund.h"\n#include "tftfund_guided.h"\n'
                       'int (*p)(tff_ctx*, uint64_t, int64_t, int64_t, int32_t, int32_t, const int32_t*, int64_t, int32_t*) = tff_sample_indices_guided_dev;\n'
                       % first)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_entry_points_refuse_a_null_context():
    build_library()
    lib = api.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "tff_robust_pose_scenes_guided_dev": (None, 0, p, p, 8, 8, 1, p, 0, 1, 10, 0, 4.0, 4, 1, 0.99, 4, p, 100, p, p, p, p, p, p, p),
        "tff_robust_pose_scenes_guided_host": (None, 0, p, p, 1, p, 0, 1, 10, 0, 4.0, 4, 1, 0.99, 4, p, 100, p, p, p, p, p, p, p),
        "tff_sample_indices_guided_dev": (None, 1, 0, 10, 7, 20, p, 100, p),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -10001, name
        assert lib.tff_last_error().decode() == "null context", name


# ---- the Python wrappers' argument errors ------------------------------------------------------------------------------------------------------------
def test_guided_argument_errors_come_before_the_library():
    torch = pytest.importorskip("torch")
    ctx = _NoLibrary()
    scenes = np.zeros((20, 6))
    off = np.array([0, 10, 20], dtype=np.int64)
    order = np.tile(np.arange(10, dtype=np.int32), 2)
    quality = np.linspace(0.0, 1.0, 20)
    bad = [
        dict(order=order, quality=quality),                                   # both
        dict(order=order[:19]), dict(quality=quality[:19]), dict(order=order.reshape(2, 10)),   # the length
        dict(order=order.astype(np.int64)), dict(order=quality), dict(quality=order),           # the dtype
        dict(order=torch.from_numpy(order)), dict(quality=torch.from_numpy(quality)), dict(order=order.tolist()),   # the device: numpy scenes want numpy
        dict(order=order, growth=0), dict(order=order, growth=api.GUIDED_MAX_GROWTH + 1), dict(quality=quality, growth=-5), dict(order=order, growth=1.5),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.robust_pose_scenes("LinearTFTPoseEstimation", scenes, off, CALM, 100, 4.0, **kw)
        with pytest.raises(ValueError):
            ctx.robust_pose_scenes("LinearFPoseEstimation", scenes, off, CALM, 100, 4.0, confidence=0.99, **kw)
    one = np.arange(20, dtype=np.int32)
    for kw in (dict(order=one, quality=quality), dict(order=one[:5]), dict(order=one.astype(np.int16)), dict(quality=one), dict(order=one, growth=0),
               dict(order=torch.from_numpy(one))):
        with pytest.raises(ValueError):
            ctx.robust_pose("LinearTFTPoseEstimation", scenes, CALM, 100, 4.0, **kw)
    # a CPU tensor is no CUDA tensor: the device path wants the ranking on the device of the scenes
    with pytest.raises(ValueError):
        ctx._check_guided(torch.zeros((20, 6), dtype=torch.float64), torch.from_numpy(one), None, 100)
    with pytest.raises(ValueError):
        ctx._check_guided(torch.zeros((20, 6), dtype=torch.float64), one, None, 100)
    with pytest.raises(ValueError):
        ctx.sample_indices_guided(1, 0, 10, 7, one, 0)                        # growth, before the device is touched
    # without a ranking growth is ignored, whatever it holds: the call goes on to the (absent) library
    with pytest.raises(AttributeError):
        ctx.robust_pose_scenes("LinearTFTPoseEstimation", scenes, off, CALM, 100, 4.0, growth=-1)


# ---- the seeds of the end-to-end case of tests/test_gpu_guided.py --------------------------------------------------------------------------------------
def test_the_use_case_seeds_separate_the_two_samplers():
    scene, calm, inlier, quality = gc.use_case()
    assert scene.shape == (gc.USE_N, 6) and inlier.sum() == gc.USE_N - int(gc.USE_SHARE * gc.USE_N)
    order = api.order_from_quality(quality, np.array([0, gc.USE_N]))
    uniform = api.sample_indices_reference(gc.USE_CALL_SEED, 0, gc.USE_N_HYP, 7, gc.USE_N)
    guided = api.sample_indices_guided_reference(gc.USE_CALL_SEED, 0, gc.USE_N_HYP, 7, order, gc.USE_GROWTH)
    assert inlier[uniform].all(axis=1).sum() == 0
    assert inlier[guided].all(axis=1).sum() >= 5
