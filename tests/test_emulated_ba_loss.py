"""
The three instances of the bundle-adjustment kernel (csrc/ba_kernel.h: no loss, Huber, Cauchy) on the lane emulator, no GPU, compiled by g++
(tests/emu/emu_ba_loss.cpp), against the numpy restatement of the loss (tests/ba_loss_oracle.py): N = 12, 40, 64, 65, 129 with 0, 2, 8, 13, 0 displaced
matches, both losses at c = 3 and c = 1.5, with and without start points.  The gate is the BA gate of tests/test_bundle_adjustment.py (status 0, the
same iter, repr_err, poses and points within 1e-9 relative) with the weights within 1e-9 absolute, after the restatement's smallest steering margin
was found to be at least 1e-10 (ba_loss_cases.gate).  The no-loss instance is the existing emulated kernel bit for bit, and the ragged chain with a
loss gives every item the bits of the fixed-N loss call on its selection (on the GPU: tests/test_gpu_ba_loss.py).

Both sides take the scale gauge out of every step (its exact value there is zero; ba_kernel.h and ba_loss_oracle.py say why): without that
the restatement did not reproduce itself to the gate, let alone the kernel it (poses 1.5e-9, weights 1e-6 at c = 1.5 px).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tft_vs_fund_amd import api

import ba_loss_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i, c_d = ctypes.c_long, ctypes.c_int, ctypes.c_double
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
LOSS_ID = {None: 0, "huber": 1, "cauchy": 2}


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_ba_loss.so")
    deps = [os.path.join(emu, f) for f in ("emu_ba_loss.cpp", "emu_primitives.h", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_ba_loss.cpp")], check=True)
    return ctypes.CDLL(out)


def _cm(Rt):
    return np.ascontiguousarray(Rt.T).reshape(12)


def _fixed(L, C, CalM, start, X0, loss, c, weight=True):
    """the emulated fixed-N call, B = 1: C (N, 6), X0 (N, 3) or None"""
    N = C.shape[0]
    C = np.ascontiguousarray(C); x0 = None if X0 is None else np.ascontiguousarray(X0)
    o = dict(Rt2=np.zeros(12), Rt3=np.zeros(12), rec=np.zeros((N, 3)), iter=np.zeros(1, dtype=np.int32), err=np.zeros(1), st=np.full(1, -7, dtype=np.int32),
             w=np.full(N, -3.0) if weight else None)
    calm, r2, r3 = np.ascontiguousarray(CalM.T).reshape(27), _cm(start[0]), _cm(start[1])     # (named: a pointer does not keep its array alive)
    rc = L.e_ba_loss_fixed(P(calm), c_l(0), P(r2), P(r3), P(C), c_l(1), c_i(N), P(x0),
                           P(o["Rt2"]), P(o["Rt3"]), P(o["rec"]), P(o["iter"]), P(o["err"]), P(o["st"]), c_i(LOSS_ID[loss]), c_d(c or 0.0), P(o["w"]))
    assert rc == 0
    return o


def _biteq(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("n,n_bad,loss,c,with_x0", bc.CASES)
def test_loss_instances_match_the_restatement(n, n_bad, loss, c, with_x0):
    L = _lib()
    sc = bc.scene(n, n_bad)
    ref = bc.restated(n, n_bad, loss, c, with_x0)
    o = _fixed(L, sc["C"], sc["CalM"], sc["start"], sc["X0"] if with_x0 else None, loss, c)
    if n_bad:                                                                 # the displaced matches are what the loss is for: six residuals of 20 px and more
        assert o["w"][sc["bad"]].max() < 0.5                                  # against three coordinates of a point leave |e| far above 2 c, where both weights are below 1 / 2
    bc.gate(ref, int(o["st"][0]), int(o["iter"][0]), float(o["err"][0]), o["Rt2"].reshape(4, 3).T, o["Rt3"].reshape(4, 3).T, o["rec"].T, o["w"],
            (n, n_bad, loss, c, with_x0))


@pytest.mark.parametrize("loss,c", (("huber", 3.0), ("cauchy", 1.5)))
def test_the_weight_output_changes_nothing_else(loss, c):
    L = _lib()
    sc = bc.scene(65, 13)
    o = _fixed(L, sc["C"], sc["CalM"], sc["start"], None, loss, c)
    o2 = _fixed(L, sc["C"], sc["CalM"], sc["start"], None, loss, c, weight=False)
    assert all(_biteq(o[k], o2[k]) for k in ("Rt2", "Rt3", "rec", "err")) and o["iter"][0] == o2["iter"][0] and o["st"][0] == o2["st"][0] == 0


@pytest.mark.parametrize("n,n_bad", bc.SIZES)
def test_no_loss_instance_is_the_existing_emulated_kernel(n, n_bad):
    """TFF_LOSS_NONE through the loss path: the bits of the emulated kernel of tests/test_bundle_adjustment.py, and weights of 1"""
    from emu import emu_build
    old = emu_build.load()
    L = _lib()
    sc = bc.scene(n, n_bad)
    for with_x0 in (False, True):
        X0 = np.ascontiguousarray(sc["X0"]) if with_x0 else None
        o = _fixed(L, sc["C"], sc["CalM"], sc["start"], X0, None, None)
        r = dict(Rt2=np.zeros(12), Rt3=np.zeros(12), rec=np.zeros((n, 3)), iter=np.zeros(1, dtype=np.int32), err=np.zeros(1), st=np.full(1, -7, dtype=np.int32))
        calm, r2, r3, C = np.ascontiguousarray(sc["CalM"].T).reshape(27), _cm(sc["start"][0]), _cm(sc["start"][1]), np.ascontiguousarray(sc["C"])
        old.emu_bundle_adjust(P(calm), c_l(0), P(r2), P(r3), P(C), c_l(1), c_i(n), P(X0), P(r["Rt2"]), P(r["Rt3"]), P(r["rec"]), P(r["iter"]), P(r["err"]), P(r["st"]))
        assert r["st"][0] == 0 and o["st"][0] == 0 and o["iter"][0] == r["iter"][0]
        assert all(_biteq(o[k], r[k]) for k in ("Rt2", "Rt3", "rec", "err"))
        assert (o["w"] == 1.0).all()
    assert L.e_ba_loss_fixed(*([None] * 14), c_i(3), c_d(1.0), None) == -1      # no fourth instance


@pytest.mark.parametrize("loss,c", (("huber", 3.0), ("cauchy", 1.5), (None, None)))
def test_ragged_items_equal_the_fixed_loss_call(loss, c):
    """the plan of tests/test_emulated_ba_ragged.py (class bounds 8, 20, 64) around the loss instances: a random mask, start points, an item with nothing
    selected and one too large; weight is NaN where deselected and over a failed item, and nothing is written beyond n_total"""
    L = _lib()
    rng = np.random.default_rng(5)
    sizes = [30, 12, 9, 40, 80, 10, 12]
    keep = [21, 1, 8, 20, 65, 0, 12]
    scs = [bc.scene(n, min(3, n // 6), seed=50 + k, focalL=38.0 + 3.0 * k) for k, n in enumerate(sizes)]
    packed, off = api.pack_ragged([np.ascontiguousarray(s["C"]) for s in scs])
    B, nt = len(sizes), packed.shape[0]
    mask = np.concatenate([np.isin(np.arange(n), rng.choice(n, k, replace=False)) * rng.choice([1, 255]) for n, k in zip(sizes, keep)]).astype(np.uint8)
    calms = np.ascontiguousarray(np.stack([s["CalM"].T.reshape(27) for s in scs]))
    r2 = np.ascontiguousarray(np.stack([_cm(s["start"][0]) for s in scs])); r3 = np.ascontiguousarray(np.stack([_cm(s["start"][1]) for s in scs]))
    x0 = np.ascontiguousarray(np.concatenate([s["X0"] for s in scs]))
    bounds = np.array([8, 20, 64], dtype=np.int32)
    for mk in (mask, None):
        w = dict(Rt2=np.full((B, 12), 5.0), Rt3=np.full((B, 12), 5.0), rec=np.full((nt, 3), 5.0), iter=np.full(B, -7, dtype=np.int32), err=np.full(B, 5.0),
                 used=np.full(B, -7, dtype=np.int32), st=np.full(B, -7, dtype=np.int32), w=np.full(nt + 4, 5.0))
        assert L.e_ba_loss_ragged(P(packed), P(off), c_l(B), c_l(nt), P(mk), P(calms), c_l(27), P(r2), P(r3), P(x0), P(bounds), P(w["Rt2"]), P(w["Rt3"]), P(w["rec"]),
                                  P(w["iter"]), P(w["err"]), P(w["used"]), P(w["st"]), c_i(LOSS_ID[loss]), c_d(c or 0.0), P(w["w"])) == 0
        assert (w["w"][nt:] == 5.0).all()
        for b in range(B):
            o0, o1 = int(off[b]), int(off[b + 1])
            sel = mk[o0:o1] != 0 if mk is not None else np.ones(o1 - o0, dtype=bool)
            m = int(sel.sum())
            if m == 0 or m > 64:
                assert w["st"][b] == (api.ST_TOO_FEW if m == 0 else api.ST_TOO_LARGE) and np.isnan(w["w"][o0:o1]).all() and np.isnan(w["Rt2"][b]).all(), b
                continue
            s = scs[b]
            ref = _fixed(L, s["C"][sel], s["CalM"], s["start"], s["X0"][sel], loss, c)
            assert w["st"][b] == ref["st"][0] and w["iter"][b] == ref["iter"][0] and w["used"][b] == m, b
            assert (ref["st"][0] == 0) == (m > 1), b                          # (one match is no problem to adjust: the solver's own failure, NaN weights)
            if ref["st"][0] != 0:
                assert np.isnan(w["w"][o0:o1]).all() and np.isnan(ref["w"]).all(), b
                continue
            assert _biteq(w["Rt2"][b], ref["Rt2"]) and _biteq(w["Rt3"][b], ref["Rt3"]) and _biteq(w["err"][b:b + 1], ref["err"]), b
            assert _biteq(w["rec"][o0:o1][sel], ref["rec"]) and _biteq(w["w"][o0:o1][sel], ref["w"]), b
            assert np.isnan(w["w"][o0:o1][~sel]).all(), b
            if loss is None:
                assert (ref["w"] == 1.0).all()
            else:
                assert (0.0 < ref["w"]).all() and (ref["w"] <= 1.0).all() and ref["w"].min() < 1.0
