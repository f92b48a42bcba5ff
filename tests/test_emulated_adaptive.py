"""
What the adaptive robust call adds to the kernels, on the lane emulator, no GPU (tests/emu/emu_adaptive.cpp compiled by g++): the sampler with a
hypothesis base and liveness against api.sample_indices_reference, the count kernel's liveness, the kernels that close a round against numpy (scatter
positions, -1 for failures and dead scenes, best, live, used, the rule at equality and under MSAC), and the early exit of the two exact-tier row kernels
on a batch with a live, a dead and a mixed wavefront.  (The whole call against the one-scene call on the GPU is tests/test_gpu_adaptive.py.)
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tft_vs_fund_amd import api
from tft_vs_fund_amd.scenes import generate_scene_batch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i, c_d, c_u = ctypes.c_long, ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_adaptive.so")
    deps = [os.path.join(emu, f) for f in ("emu_adaptive.cpp", "emu_primitives.h", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_adaptive.cpp")], check=True)
    return ctypes.CDLL(out)


SIZES = [5, 9, 16, 61, 40]
S = len(SIZES)
MASK64 = (1 << 64) - 1


def _synth(n, seed):
    C, CalM, Rt0, _ = generate_scene_batch(1, n, noise=0.5, seed=seed)
    return np.ascontiguousarray(C[0]), np.ascontiguousarray(CalM), Rt0


ITEMS = [_synth(n, 3 + k) for k, n in enumerate(SIZES)]
PACKED, OFF = api.pack_ragged([a for a, _, _ in ITEMS])
CALMS = np.ascontiguousarray(np.stack([c.T.reshape(27) for _, c, _ in ITEMS]))
NTOT = PACKED.shape[0]


def _set(n_min, off=OFF, ns_max=61):
    return (P(PACKED), P(off), c_l(S), c_l(NTOT), c_i(ns_max), c_i(n_min), P(CALMS), c_l(27))


def test_sampler_addresses_a_round_and_skips_dead_scenes():
    L = _lib()
    n, seed = 7, (1 << 64) - 2                                                # the seed wraps at scene 2
    live = np.array([1, 1, 0, 1, 1], dtype=np.int32)
    for base, length, first in ((0, 8, 0), (8, 8, 0), (16, 13, 5), (1 << 20, 4, 3)):   # (13: a last round of odd length; first: a chunk that starts inside scene 0)
        B = S * length - first
        out = np.full((B, n), -7, dtype=np.int32); calm_out = np.zeros((B, 27))
        L.a_sample(*_set(n), c_u(seed), c_l(first), c_l(B), c_l(length), c_i(n), P(out), P(calm_out), c_l(base), P(live))
        for b in range(B):
            s, i = divmod(first + b, length)
            if SIZES[s] < n or not live[s]:
                assert (out[b] == -1).all(), (base, b)
            else:
                assert np.array_equal(out[b], api.sample_indices_reference((seed + s) & MASK64, base + i, 1, n, SIZES[s])[0] + OFF[s]), (base, b)
            assert np.array_equal(calm_out[b], CALMS[s])
    # no liveness array and base 0: the fixed call's sampler
    out = np.zeros((S * 6, n), dtype=np.int32); calm_out = np.zeros((S * 6, 27))
    L.a_sample(*_set(n), c_u(5), c_l(0), c_l(S * 6), c_l(6), c_i(n), P(out), P(calm_out), c_l(0), None)
    for b in range(S * 6):
        s, h = divmod(b, 6)
        want = -1 if SIZES[s] < n else api.sample_indices_reference(5 + s, h, 1, n, SIZES[s])[0] + OFF[s]
        assert np.array_equal(out[b], np.broadcast_to(want, (n,)))


def _cm(Rt):
    return np.ascontiguousarray(Rt.T).reshape(12)


def test_count_kernel_skips_a_dead_scenes_segment():
    L = _lib()
    per = 5; B = S * per
    Rt2 = np.stack([_cm(ITEMS[b // per][2][0]) for b in range(B)]); Rt3 = np.stack([_cm(ITEMS[b // per][2][1]) for b in range(B)])
    ref = np.full(B, -9, dtype=np.int32); got = np.full(B, -9, dtype=np.int32)
    L.a_count(*_set(7), P(Rt2), P(Rt3), c_l(0), c_l(B), c_l(per), c_l(16), c_d(4.0), P(ref), c_i(6 * 61), None)
    live = np.array([1, 0, 1, 0, 1], dtype=np.int32)
    L.a_count(*_set(7), P(Rt2), P(Rt3), c_l(0), c_l(B), c_l(per), c_l(16), c_d(4.0), P(got), c_i(6 * 61), P(live))
    assert (ref[:per] == -1).all() and (ref[per:] > 0).all()                  # scene 0 is too small; the ground-truth poses have inliers
    for s in range(S):
        seg = slice(s * per, (s + 1) * per)
        assert np.array_equal(got[seg], ref[seg] if live[s] else np.full(per, -1)), s


def test_round_kernels_against_numpy():
    """three rounds of 4, 4 and 5 hypotheses (n_hyp = 13) with made-up counts; scene 0 is invalid (5 < 7 matches), scene 1 (9 matches) never succeeds,
    scene 2 (16) meets qmin exactly in round 1, scene 3 (61) stops in round 2, scene 4 (40) never reaches the threshold"""
    L = _lib()
    n_hyp, ends, n = 13, [4, 8, 13], 7
    for msac in (False, True):
        units = 64 if msac else 1
        w = np.float64(3) / np.float64(16); q1 = w
        for _ in range(n - 1):
            q1 = q1 * w                                                       # scene 2's q with 3 inliers: the threshold of round 1, met with equality
        qmin = [float(q1), float(q1) * 0.9, 1e-3]
        rng = np.random.default_rng(4 + msac)
        live = np.full(S, -5, dtype=np.int32); best = np.full(S, 77, dtype=np.uint64); used = np.full(S, -5, dtype=np.int32)
        counts = np.full(S * n_hyp, -1, dtype=np.int32)
        L.a_round_init(*_set(n), P(live), P(best), P(used))
        assert live.tolist() == [0, 1, 1, 1, 1] and (best == 0).all() and (used == 0).all()
        ref_counts = counts.copy(); ref_live = live.copy(); ref_used = used.copy(); ref_best = np.full(S, -1)
        e_prev = 0
        for r, e_end in enumerate(ends):
            length = e_end - e_prev
            dense = rng.integers(0, 3 * units, (S, length)).astype(np.int32)  # (at most 2 inliers: 0 < q < qmin unless set below)
            status = (rng.random((S, length)) < 0.3).astype(np.int32) * 3
            status[1] = 5                                                     # scene 1: every hypothesis fails
            if r == 0:
                dense[2, 1] = 3 * units + (units - 1); status[2, 1] = 0       # 3 inliers exactly (MSAC: the largest score that still divides to 3)
                dense[2, 2] = 9 * units; status[2, 2] = 2                     # a failed hypothesis does not count, whatever it holds
            if r == 1:
                dense[3, 0] = 40 * units; status[3, 0] = 0                    # (40 / 61)^7 = 0.05: far above qmin
            dense[~ref_live.astype(bool)] = -1                                # what the count kernel writes for a scene that is not live
            for first, B in ((0, 7), (7, S * length - 7)):                    # two chunks, the cut inside a scene
                d = np.ascontiguousarray(dense.reshape(-1)[first:first + B]); st = np.ascontiguousarray(status.reshape(-1)[first:first + B])
                L.a_round_scatter(P(d), P(st), c_l(first), c_l(B), c_l(length), c_l(e_prev), c_l(n_hyp), P(live), P(best), P(counts))
            L.a_round_close(*_set(n), P(live), P(best), P(used), c_l(e_end), c_d(qmin[r]), c_i(n), c_i(units))
            for s in range(S):
                if not ref_live[s]:
                    continue
                marked = np.where(status[s] != 0, -1, dense[s])
                ref_counts[s * n_hyp + e_prev: s * n_hyp + e_end] = marked
                ref_best[s] = max(ref_best[s], int(marked.max()))
                ref_used[s] = e_end
                if api.adaptive_stop(ref_best[s], SIZES[s], n, qmin[r], msac=msac):
                    ref_live[s] = 0
            assert np.array_equal(counts, ref_counts), (msac, r)
            assert np.array_equal(best.astype(np.int64) - 1, ref_best), (msac, r)
            assert np.array_equal(live, ref_live) and np.array_equal(used, ref_used), (msac, r)
            e_prev = e_end
        assert used.tolist() == [0, 13, 4, 8, 13] and live.tolist() == [0, 1, 0, 0, 1]
        assert (counts[:n_hyp] == -1).all() and (counts[n_hyp:2 * n_hyp] == -1).all()           # the invalid scene, the scene without a success
        assert (counts[2 * n_hyp + 4:3 * n_hyp] == -1).all() and (counts[3 * n_hyp + 8:4 * n_hyp] == -1).all()   # never drawn
        assert best[1] == 0


@pytest.mark.parametrize("linear_f", [0, 1])
def test_exact_row_kernels_leave_early_on_a_dead_wavefront(linear_f):
    """12 sampled rows, three wavefronts of four: all live | all dead | two live, two dead.  Dead rows: ST_TOO_FEW and NaN; live rows: the bits of the same
    hypotheses in an all-live batch"""
    L = _lib()
    n = 8 if linear_f else 7
    B = 12
    scene_of = [3, 3, 4, 4, 3, 3, 3, 3, 4, 4, 3, 3]
    idx_all = np.zeros((B, n), dtype=np.int32)
    for b in range(B):
        idx_all[b] = api.sample_indices_reference(11 + scene_of[b], b, 1, n, SIZES[scene_of[b]])[0] + OFF[scene_of[b]]
    calm = np.ascontiguousarray(CALMS[scene_of])
    dead = np.array([0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1], dtype=bool)
    idx = idx_all.copy(); idx[dead] = -1

    def run(ix):
        Rt2 = np.full((B, 12), 7.0); Rt3 = np.full((B, 12), 7.0); T = np.full((B, 27), 7.0); st = np.full(B, -3, dtype=np.int32)
        L.a_rows_exact(c_i(linear_f), P(PACKED), c_i(NTOT), P(calm), P(np.ascontiguousarray(ix)), c_l(B), c_i(n), P(Rt2), P(Rt3), P(T), P(st))
        return Rt2, Rt3, T, st
    ref = run(idx_all)
    got = run(idx)
    assert (ref[3] == 0).sum() >= 8                                           # (most hypotheses succeed: the comparison below is of poses, not of sentinels)
    assert (got[3][dead] == api.ST_TOO_FEW).all()
    for a in got[:3]:
        assert np.isnan(a[dead]).all()
    for a, r in zip(got, ref):
        assert np.array_equal(a[~dead].view(np.int64) if a.dtype == np.float64 else a[~dead], r[~dead].view(np.int64) if r.dtype == np.float64 else r[~dead])
