"""
The ragged chain of OptimFPoseEstimation on the lane emulator, no GPU: the plan of csrc/ragged_kernel.h with OptimF's two additions (the three ranges
of the refinement, the exact range published on the retry list) and the <RAGGED> forms of k_optimf_linear_rows, k_optimf_refine, k_optimf_finish_rows and
k_f_pose<true, 1>, compiled by g++ (tests/emu/emu_optimf_ragged.cpp).  The storage bounds of the refinement are passed in as (16, 33) instead of the
library's (tff_optim_f_ragged_bounds), so items of 12 .. 64 matches reach all three launch classes: observations staged in LDS, estimates in LDS,
estimates in a global slice.  Items of 7, 8, 11, 12, 13, 16, 17, 33 and 64 matches, five of them with 13 (a slot of four and a slot with three padding
entries), a CalM per item, a decreasing offset.  References: numpy for the plan; the emulated fixed-N chain on each item alone, bit for bit;
oracle.tft_oracle.OptimFPoseEstimation at 1e-8 and the same `iter` (the gate of tests/test_emulated_kernels.py::test_optim_f_staged_matches_fused_and_oracle)
for every item of 8 matches and more, the exact range (8, 11) included; the item of 7 has no pose to compare (ST_TOO_FEW, NaN).  The figures are
printed before they are asserted (pytest -s).
(Bit-identity with the fixed-N entry point on the GPU is tests/test_gpu_ragged_optimf.py.)
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import rel_err_T, rel_err
from oracle import tft_oracle as O
from tft_vs_fund_amd import api
from tft_vs_fund_amd.scenes import generate_scene_batch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i = ctypes.c_long, ctypes.c_int
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
SPLIT, STAGE_UPTO, XI_UPTO = 12, 16, 33
SIZES = [17, 13, 7, 13, 64, 8, 13, 11, 33, 13, 16, 12, 13]                       # (no slot of the list holds the item of the same index)


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_optimf_ragged.so")
    deps = [os.path.join(emu, f) for f in ("emu_optimf_ragged.cpp", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_optimf_ragged.cpp")], check=True)
    return ctypes.CDLL(out)


def _biteq(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def run():
    L = _lib()
    items, calms = [], []
    for k, n in enumerate(SIZES):
        C, CalM, _, _ = generate_scene_batch(1, n, noise=1.0, seed=50 + k, focalL=40.0 + 2.0 * k)
        items.append(np.ascontiguousarray(C[0])); calms.append(np.ascontiguousarray(CalM.T).reshape(27))
    calms = np.ascontiguousarray(np.stack(calms))
    assert all(not np.array_equal(calms[0], c) for c in calms[1:])
    packed, off = api.pack_ragged(items)
    B, nt, n_max = len(items), packed.shape[0], max(SIZES)
    slots = B + 3 * min(B, n_max + 1)
    o = dict(Rt2=np.full((B, 12), 5.0), Rt3=np.full((B, 12), 5.0), T=np.full((B, 27), 5.0), rec=np.full((nt, 3), 5.0), iter=np.full(B, -7, dtype=np.int32),
             status=np.full(B, -7, dtype=np.int32), route=np.full(10, -7, dtype=np.int32), list=np.full(slots, -7, dtype=np.int32))
    o["listed"] = L.e_optimf_ragged(P(packed), P(off), c_l(B), c_i(n_max), P(calms), c_l(27), c_i(SPLIT), c_i(STAGE_UPTO), c_i(XI_UPTO), P(o["Rt2"]),
                                    P(o["Rt3"]), P(o["T"]), P(o["rec"]), P(o["iter"]), P(o["status"]), P(o["route"]), P(o["list"]))
    return L, items, calms, packed, off, o


def _fixed(L, item, calm):
    n = item.shape[0]
    f = dict(Rt2=np.full(12, 5.0), Rt3=np.full(12, 5.0), T=np.full(27, 5.0), rec=np.full((n, 3), 5.0), iter=np.full(1, -7, dtype=np.int32),
             status=np.full(1, -7, dtype=np.int32))
    L.e_optimf_fixed(P(item), P(calm), c_l(0), c_l(1), c_i(n), c_i(n < SPLIT), c_i(n <= STAGE_UPTO), c_i(n > XI_UPTO), P(f["Rt2"]), P(f["Rt3"]), P(f["T"]),
                     P(f["rec"]), P(f["iter"]), P(f["status"]))
    return f


def test_plan(run):
    """the slot list is sorted by n in slots of four, padded with -1; the five ranges are where numpy puts them"""
    _, items, _, _, _, o = run
    ns = np.array(SIZES)
    padded = lambda sel: int(sum((np.sum(ns == n) + 3) & ~3 for n in np.unique(ns[sel])))
    mid = padded(ns < SPLIT); c0 = mid + padded((ns >= SPLIT) & (ns <= STAGE_UPTO)); c1 = c0 + padded((ns > STAGE_UPTO) & (ns <= XI_UPTO))
    total = padded(ns >= 0)
    assert o["route"].tolist() == [0, mid, mid, total, mid, c0, c0, c1, c1, total]
    lst = o["list"][:total]
    for s in range(0, total, 4):
        e = lst[s:s + 4]
        assert e[0] >= 0 and all(x == -1 or ns[x] == ns[e[0]] for x in e)
        assert all(e[k] == -1 for k in range(4) if k > 0 and e[k - 1] == -1)
    assert sorted(lst[lst >= 0].tolist()) == list(range(len(SIZES)))
    first = [ns[lst[s]] for s in range(0, total, 4)]
    assert first == sorted(first)
    assert (lst[np.arange(total) < len(SIZES)] != np.arange(min(total, len(SIZES)))).all()
    assert o["listed"] == int(np.sum(ns < SPLIT))                               # the exact range, and nothing the staged kernels flagged


def test_bitwise_equals_the_fixed_n_chain_and_oracle(run):
    L, items, calms, packed, off, o = run
    for b, item in enumerate(items):
        n = item.shape[0]
        f = _fixed(L, item, calms[b])
        assert o["status"][b] == f["status"][0] and o["iter"][b] == f["iter"][0], (b, n, o["status"][b], f["status"][0])
        assert o["status"][b] == (api.ST_TOO_FEW if n < 8 else 0), (b, n)
        for k in ("Rt2", "Rt3", "T"):
            assert _biteq(o[k][b], f[k]), (b, n, k)
        assert _biteq(o["rec"][off[b]:off[b + 1]], f["rec"]), (b, n)
        if n < 8:
            assert np.isnan(o["T"][b]).all() and np.isnan(o["rec"][off[b]:off[b + 1]]).all()
        if n >= 12:
            assert o["iter"][b] >= 2                                            # (the refinement ran)
        if n >= 8:
            R2, R3, Rec, T, it = O.OptimFPoseEstimation(item.T.copy(), calms[b].reshape(3, 9).T.copy())
            print("n = %2d iter %d / %d  T %.2e  Rt2 %.2e  Rt3 %.2e  Reconst %.2e" % (
                n, int(it), int(o["iter"][b]), rel_err_T(o["T"][b].reshape(3, 3, 3).transpose(2, 1, 0), T), rel_err(o["Rt2"][b].reshape(4, 3).T, R2),
                rel_err(o["Rt3"][b].reshape(4, 3).T, R3), rel_err(o["rec"][off[b]:off[b + 1]].T, Rec)))
            assert int(it) == int(o["iter"][b]), (b, n)
            assert rel_err_T(o["T"][b].reshape(3, 3, 3).transpose(2, 1, 0), T) < 1e-8 and rel_err(o["Rt2"][b].reshape(4, 3).T, R2) < 1e-8
            assert rel_err(o["Rt3"][b].reshape(4, 3).T, R3) < 1e-8 and rel_err(o["rec"][off[b]:off[b + 1]].T, Rec) < 1e-8


def test_bad_offsets_leave_the_neighbours_alone(run):
    """item 1 ends before it starts: ST_BAD_OFFSETS, NaN poses, no Reconst; the others equal the clean batch"""
    L, items, calms, packed, off, o = run
    B, nt, n_max = 4, int(off[4]), max(SIZES[:4])
    bad = off[:5].copy(); bad[2] = off[1] - 1                                   # item 2 now reads one correspondence more
    slots = B + 3 * min(B, n_max + 1)
    w = dict(Rt2=np.full((B, 12), 5.0), Rt3=np.full((B, 12), 5.0), T=np.full((B, 27), 5.0), rec=np.full((nt, 3), 5.0), iter=np.full(B, -7, dtype=np.int32),
             status=np.full(B, -7, dtype=np.int32), route=np.full(10, -7, dtype=np.int32), list=np.full(slots, -7, dtype=np.int32))
    L.e_optimf_ragged(P(packed), P(bad), c_l(B), c_i(n_max), P(calms), c_l(27), c_i(SPLIT), c_i(STAGE_UPTO), c_i(XI_UPTO), P(w["Rt2"]), P(w["Rt3"]), P(w["T"]),
                      P(w["rec"]), P(w["iter"]), P(w["status"]), P(w["route"]), P(w["list"]))
    assert w["status"][1] == api.ST_BAD_OFFSETS and np.isnan(w["T"][1]).all() and np.isnan(w["Rt2"][1]).all() and w["iter"][1] == 0
    for b in (0, 3):
        assert w["status"][b] == o["status"][b] and w["iter"][b] == o["iter"][b]
        for k in ("Rt2", "Rt3", "T"):
            assert _biteq(w[k][b], o[k][b]), (b, k)
        assert _biteq(w["rec"][off[b]:off[b + 1]], o["rec"][off[b]:off[b + 1]]), b
    assert (w["rec"][off[1]:off[2] - 1] == 5.0).all()                            # nobody's range
