"""
The kernels of the guided (PROSAC) sampler on the lane emulator, no GPU (tests/emu/emu_guided.cpp compiled by g++): the pool-table kernel against
api.guided_pool_ends and the sampler against api.sample_indices_guided_reference, index for index, on scenes of 5 (too few), 7, 8, 61 and 400
correspondences packed together -- with a hypothesis base, a dead scene, the re-draw from selection keys, the per-row CalM copy, and a ranking with one
entry out of range.  (The whole call against the one-scene call on the GPU is tests/test_gpu_guided.py.)
"""
import ctypes
import os
import subprocess

import numpy as np

from tft_vs_fund_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i, c_u = ctypes.c_long, ctypes.c_int, ctypes.c_ulonglong
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_guided.so")
    deps = [os.path.join(emu, f) for f in ("emu_guided.cpp", "emu_primitives.h", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_guided.cpp")], check=True)
    return ctypes.CDLL(out)


SIZES = [5, 7, 8, 61, 400]
S = len(SIZES)
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
NTOT = int(OFF[-1])
MASK64 = (1 << 64) - 1
CALMS = np.arange(S * 27, dtype=np.float64).reshape(S, 27)
RNG = np.random.default_rng(17)
ORDER = np.concatenate([RNG.permutation(n) for n in SIZES]).astype(np.int32)


def _table(L, m, growth, blocks=S):
    ends = np.full(NTOT, -7, dtype=np.int32)
    L.g_ends(P(OFF), c_l(S), c_l(NTOT), c_i(400), c_i(m), c_l(growth), P(ends), c_i(blocks))
    return ends


def _row(seed, s, h, m, growth, order=ORDER):
    return api.sample_indices_guided_reference((seed + s) & MASK64, h, 1, m, order[OFF[s]:OFF[s + 1]], growth)[0]


def test_table_kernel_is_guided_pool_ends():
    L = _lib()
    for m, growth, blocks in ((7, 200000, S), (8, 64, 2), (7, 1, 1), (8, api.GUIDED_MAX_GROWTH, 3)):
        ends = _table(L, m, growth, blocks)
        for s, n in enumerate(SIZES):
            got = ends[OFF[s]:OFF[s + 1]]
            if n < m:
                assert (got == -7).all(), (m, s)                              # an invalid scene: nothing is written
            else:
                assert np.array_equal(got, api.guided_pool_ends(n, m, growth)[1:]), (m, growth, s)


def test_sampler_is_the_twin_for_rounds_keys_and_dead_scenes():
    L = _lib()
    m, growth, seed = 7, 300, (1 << 64) - 2                                   # the seed wraps at scene 2; growth 300: scenes 1 .. 3 reach the uniform draw
    ends = _table(L, m, growth)
    live = np.array([1, 1, 0, 1, 1], dtype=np.int32)
    for base, length, first, lv in ((0, 40, 0, None), (40, 37, 11, live), (300, 16, 3, live), ((1 << 32) - 20, 8, 0, None)):
        B = S * length - first
        out = np.full((B, m), -7, dtype=np.int32); calm_out = np.zeros((B, 27))
        L.g_sample(P(OFF), c_l(S), c_l(NTOT), c_i(400), c_i(m), P(CALMS), c_l(27), c_u(seed), c_l(first), None, c_l(B), c_l(length), P(out),
                   P(calm_out), c_l(base), P(lv), P(ends), P(ORDER))
        for b in range(B):
            s, i = divmod(first + b, length)
            if SIZES[s] < m or (lv is not None and not lv[s]):
                assert (out[b] == -1).all(), (base, b)
            else:
                assert np.array_equal(out[b], _row(seed, s, base + i, m, growth) + OFF[s]), (base, b)
            assert np.array_equal(calm_out[b], CALMS[s])
    # the re-draw of K = 3 candidates per scene from their selection keys: the same function of h; key 0 (no candidate) is hypothesis 0
    K = 3
    hyps = np.array([[0, 1, 2], [0, 5, 299], [7, 400, 12], [3, 60, 5000], [1, 250, 100000]], dtype=np.uint64)
    keys = ((np.uint64(5) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - hyps)).reshape(-1)
    keys[4] = 0
    hyps[1, 1] = 0
    out = np.full((S * K, m), -7, dtype=np.int32)
    L.g_sample(P(OFF), c_l(S), c_l(NTOT), c_i(400), c_i(m), P(CALMS), c_l(0), c_u(seed), c_l(0), P(keys), c_l(S * K), c_l(K), P(out), None, c_l(0), None,
               P(ends), P(ORDER))
    for r in range(S * K):
        s, k = divmod(r, K)
        want = np.full(m, -1) if SIZES[s] < m else _row(seed, s, int(hyps[s, k]), m, growth) + OFF[s]
        assert np.array_equal(out[r], want), r


def test_an_order_entry_out_of_range_gives_minus_one_rows_and_nothing_else():
    L = _lib()
    m, growth, seed, n_hyp = 8, 64, 9, 200
    ends = _table(L, m, growth)
    rows_hit = 0
    for bad_value in (-1, 61, 1 << 30):
        order = ORDER.copy()
        order[OFF[3] + 20] = bad_value                                        # rank 20 of the scene of 61 now points outside it
        out = np.full((S * n_hyp, m), -7, dtype=np.int32)
        L.g_sample(P(OFF), c_l(S), c_l(NTOT), c_i(400), c_i(m), P(CALMS), c_l(0), c_u(seed), c_l(0), None, c_l(S * n_hyp), c_l(n_hyp), P(out), None,
                   c_l(0), None, P(ends), P(order))
        clean = np.full_like(out, -7)
        L.g_sample(P(OFF), c_l(S), c_l(NTOT), c_i(400), c_i(m), P(CALMS), c_l(0), c_u(seed), c_l(0), None, c_l(S * n_hyp), c_l(n_hyp), P(clean), None,
                   c_l(0), None, P(ends), P(ORDER))
        draws = clean[3 * n_hyp:4 * n_hyp] == OFF[3] + ORDER[OFF[3] + 20]     # the hypotheses that draw rank 20, by the clean run
        hit = draws.any(axis=1)
        assert 0 < hit.sum() < n_hyp
        rows_hit += int(hit.sum())
        want = clean.copy()
        want[3 * n_hyp:4 * n_hyp][hit] = -1
        assert np.array_equal(out, want), bad_value
        for h in np.nonzero(hit)[0][:3]:                                      # ... and by the twin
            assert (_row(seed, 3, int(h), m, growth, order) == -1).all()
    assert rows_hit > 0


def test_one_scene_kernel_is_the_twin():
    L = _lib()
    for Ns, m, growth, first in ((7, 7, 1, 0), (61, 7, 200000, (1 << 32) - 3), (400, 8, 64, 0)):
        order = np.random.default_rng(Ns).permutation(Ns).astype(np.int32)
        ends = np.ascontiguousarray(api.guided_pool_ends(Ns, m, growth)[1:])
        out = np.zeros((300, m), dtype=np.int32)
        L.g_sample_one(c_u(77), c_l(first), c_l(300), c_i(m), c_i(Ns), P(out), P(ends), P(order))
        assert np.array_equal(out, api.sample_indices_guided_reference(77, first, 300, m, order, growth)), (Ns, m, growth)


def test_guided_kernel_is_the_uniform_one_beyond_the_table_and_for_dead_and_invalid_scenes():
    """k_scenes_sample_guided and k_scenes_sample share their row function: with the identity ranking the two kernels agree index for index wherever the
    guided draw is the uniform one (hypothesis h + 1 beyond ends[N]), and for every row of a dead or an invalid scene (-1 from both); the CalM copies agree
    everywhere.  Two scenes of 9 and 7 correspondences, n = 7, growth = 1, 12 hypotheses per scene."""
    L = _lib()
    sizes, m, growth, n_hyp, seed = [9, 7], 7, 1, 12, 2024
    off = np.array([0, 9, 16], dtype=np.int64)
    ident = np.concatenate([np.arange(n) for n in sizes]).astype(np.int32)
    calms = np.arange(2 * 27, dtype=np.float64).reshape(2, 27)
    ends = np.full(16, -7, dtype=np.int32)
    L.g_ends(P(off), c_l(2), c_l(16), c_i(9), c_i(m), c_l(growth), P(ends), c_i(2))
    last = [int(api.guided_pool_ends(n, m, growth)[-1]) for n in sizes]      # ends[N] per scene
    assert [int(ends[8]), int(ends[15])] == last and all(0 < e < n_hyp for e in last)
    B = 2 * n_hyp
    for ns_max, live, quiet in ((9, None, ()), (9, np.array([0, 1], dtype=np.int32), (0,)), (9, np.array([1, 0], dtype=np.int32), (1,)), (8, None, (0,))):
        got = np.full((B, m), -7, dtype=np.int32); want = np.full((B, m), -7, dtype=np.int32)
        cg = np.zeros((B, 27)); cu = np.zeros((B, 27))
        L.g_sample(P(off), c_l(2), c_l(16), c_i(ns_max), c_i(m), P(calms), c_l(27), c_u(seed), c_l(0), None, c_l(B), c_l(n_hyp), P(got), P(cg), c_l(0),
                   P(live), P(ends), P(ident))
        L.g_sample_uniform(P(off), c_l(2), c_l(16), c_i(ns_max), c_i(m), P(calms), c_l(27), c_u(seed), c_l(0), None, c_l(B), c_l(n_hyp), P(want), P(cu),
                           c_l(0), P(live))
        assert np.array_equal(cg, cu) and np.array_equal(cu, np.repeat(calms, n_hyp, axis=0))
        for s in range(2):
            rows = slice(s * n_hyp, (s + 1) * n_hyp)
            if s in quiet:                                                    # dead (live[s] == 0) or invalid (9 > ns_max = 8): a row of -1 from both
                assert (got[rows] == -1).all() and (want[rows] == -1).all(), (ns_max, s)
            else:                                                             # beyond the table: the uniform draw, through the identity ranking
                assert np.array_equal(got[rows][last[s]:], want[rows][last[s]:]), (ns_max, s)
                assert (want[rows] >= off[s]).all() and (want[rows] < off[s + 1]).all()
